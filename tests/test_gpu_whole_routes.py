"""The value half of tests/test_whole_routes.py, on the product build (which has no launch log): at 401 nt, the first length
past the window limit, every Python-level caller of a whole-record fold returns exactly (==) what the direct Engine call gives
that the route table names for it ("Routes of the whole-record folds"): energies, structures, and the
partition-function dicts under the same hint.  Spans 100 and 101 lie either side of the facade's rule 4 span <= L."""
import random
import statistics

import numpy as np
import pytest

from scanfold_amd import RNA, _lib, functions
from scanfold_amd import scanfold as sfd
from long_util import rand_seq

pytestmark = pytest.mark.gpu

L = _lib.SF_MAX_W + 1
SEQ = rand_seq(np.random.default_rng(401), L)
SHORT = rand_seq(np.random.default_rng(120), 120)
CONS1 = "." * 10 + "(" + "." * 19 + ")" + "." * (L - 31)
CONS2 = "." * 5 + "x" + "." * (L - 6)
PF_KEYS = ("dG", "mean_bp_dist", "centroid", "centroid_dist")


@pytest.fixture(autouse=True)
def shared_engine(gpu_engine, monkeypatch):
    monkeypatch.setattr(_lib, "_engine", gpu_engine)
    RNA._check_md(None)
    yield
    RNA._check_md(None)
    assert gpu_engine.max_bp_span == 0 and gpu_engine.md_span == 0 and gpu_engine.params.temperature == 37.0


def under(eng, span, call):
    """call() with `span` resident, set beside the facade"""
    eng.set_max_bp_span(span)
    try:
        return call()
    finally:
        eng.set_max_bp_span(0)


def kcal(dcal):
    return float(np.float32(dcal) / np.float32(100.0))


@pytest.mark.parametrize("span,entry", [(0, "fold_long"), (100, "fold_banded"), (101, "fold_long")])
@pytest.mark.parametrize("cons", [None, CONS1], ids=["free", "constrained"])
def test_facade_mfe(gpu_engine, span, entry, cons):
    m = RNA.md()
    m.max_bp_span = span or -1
    fc = RNA.fold_compound(SEQ, m)
    if cons:
        fc.hc_add_from_db(cons)
    db, e = fc.mfe()
    assert (gpu_engine.max_bp_span, gpu_engine.md_span) == (span, span)
    RNA._check_md(None)
    want_e, want_db = under(gpu_engine, span, lambda: getattr(gpu_engine, entry)(SEQ, cons))
    assert (db, e) == (want_db, kcal(want_e))


def test_energies(gpu_engine):
    got = under(gpu_engine, 100, lambda: functions.energies([SEQ, SHORT, SEQ[::-1]]))  # full tables whatever span is resident
    long_e = under(gpu_engine, 100, lambda: gpu_engine.fold_long_batch([SEQ, SEQ[::-1]]))
    short_e = under(gpu_engine, 100, lambda: gpu_engine.mfe_batch([SHORT]))
    assert got == [kcal(long_e[0]), kcal(short_e[0]), kcal(long_e[1])]


def test_rna_refold(gpu_engine, tmp_path):
    (tmp_path / "c.txt").write_text(SEQ + "\n" + CONS1 + "\n")
    structure, centroid, mfe, ed = functions.rna_refold(SEQ, 37, str(tmp_path / "c.txt"))
    e, db = gpu_engine.fold_long(SEQ, CONS1)
    r = gpu_engine.pf_long(SEQ, CONS1, mfe_hint=e)
    assert (structure, centroid, mfe, ed) == (db, r["centroid"], kcal(e), round(r["mean_bp_dist"], 2))


def dbn_files(tmp_path):
    base = str(tmp_path / "rec")
    for tag, line in (("no_filter", "." * L), ("-1", CONS1), ("-2", CONS2)):
        with open(base + ".ScanFold." + tag + ".dbn", "w") as w:
            w.write(">rec\n" + SEQ + "\n" + line + "\n")
    return base


LABELS = ("Global Full", "Refolded with -1 constraints", "Refolded with -2 constraints")


@pytest.mark.parametrize("case,kw,fold,pf", [
    ("span=0", dict(), "fold_long", None),
    ("span=60", dict(span=60), "fold_banded", None),
    ("ensemble", dict(ensemble=True), "fold_long", "pf_long_batch"),
    ("ensemble under a span", dict(ensemble=True, span=60), "fold_banded", "pf_long_batch"),
    ("ensemble, no batch", dict(ensemble=True), "fold_long", "pf_long"),
    ("ensemble_banded", dict(span=60, ensemble_banded=True), "fold_banded", "pf_banded"),
])
def test_global_refold(gpu_engine, monkeypatch, tmp_path, case, kw, fold, pf):
    eng = gpu_engine
    if case == "ensemble, no batch":
        monkeypatch.setattr(eng, "has_pf_long_batch", lambda: False)
    base = dbn_files(tmp_path)
    span = kw.get("span", 0)
    params0 = eng.params
    sfd.global_refold(SEQ, "rec", base, 37, **kw)
    assert eng.params is params0 and eng.max_bp_span == 0
    cons = [None, CONS1, CONS2]
    folds = under(eng, span, lambda: [getattr(eng, fold)(SEQ, c) for c in cons])
    tail = " span=%d" % span if span else ""
    want = "".join(">rec\t%s MFE=%s%s\n%s\n%s\n" % (label, str(kcal(e)), tail, SEQ, db) for label, (e, db) in zip(LABELS, folds))
    assert open(base + ".AllDBN-global_refold.txt").read() == want
    if pf is None:
        return
    hints = [int(round(kcal(e) * 100)) for e, _ in folds]
    if pf == "pf_long_batch":
        ens = under(eng, span, lambda: eng.pf_long_batch([SEQ] * 3, cons, hints))
    else:
        ens = under(eng, span, lambda: [getattr(eng, pf)(SEQ, c, mfe_hint=h) for c, h in zip(cons, hints)])
    want = "".join(">rec\t%s ensemble dG=%.2f ED=%.2f centroid distance=%.2f%s\n%s\n%s\n"
                   % (label, r["dG"], r["mean_bp_dist"], r["centroid_dist"], tail if pf == "pf_banded" else "", SEQ, r["centroid"])
                   for label, r in zip(LABELS, ens))
    assert open(base + ".AllDBN-global_refold.ensemble.txt").read() == want


def test_the_executors_return_the_engine_calls_results(gpu_engine):
    """whole.fold / whole.pf / whole.pf_rows against the Engine methods, dict for dict (the driver's files round to two places)"""
    from scanfold_amd import whole
    eng = gpu_engine
    e, db = eng.fold_long(SEQ, CONS1)
    assert whole.fold(eng, SEQ, CONS1, whole.NEVER) == (e, db)
    one = eng.pf_long(SEQ, CONS1, mfe_hint=e)
    assert whole.pf(eng, SEQ, CONS1, e, whole.NEVER) == one
    rows = whole.pf_rows(eng, SEQ, [None, CONS1], [None, e], whole.NEVER)
    assert rows == eng.pf_long_batch([SEQ] * 2, [None, CONS1], [None, e])
    assert {k: rows[1][k] for k in PF_KEYS} == one  # (a batch row is pf_long's bit for bit)
    banded = under(eng, 60, lambda: (whole.fold(eng, SEQ, CONS1, whole.ALWAYS), eng.fold_banded(SEQ, CONS1),
                                     whole.pf(eng, SEQ, CONS1, e, whole.ALWAYS), eng.pf_banded(SEQ, CONS1, mfe_hint=e)))
    assert banded[0] == banded[1] and banded[2] == banded[3]


@pytest.mark.parametrize("span,entry", [(0, "fold_long_batch"), (60, "fold_banded_batch")])
def test_global_zscore(gpu_engine, tmp_path, span, entry):
    eng = gpu_engine
    state = random.getstate()
    params0 = eng.params
    sfd.global_zscore(SEQ, "rec", str(tmp_path / "rec"), 37, 2, "mono", seed=3, span=span)
    assert random.getstate() == state and eng.params is params0 and eng.max_bp_span == 0
    random.seed(3)
    rows = [SEQ] + functions.scramble(SEQ, 2, "mono")
    random.setstate(state)
    E = [kcal(v) for v in under(eng, span, lambda: getattr(eng, entry)(rows))]
    row = ["rec", str(L), "37", "2", "mono"] + [str(round(x, 2)) for x in (
        E[0], statistics.mean(E[1:]), statistics.stdev(E[1:]), functions.zscore_function(E, 2), functions.pvalue_function(E, 2))]
    header = sfd.GLOBAL_ZSCORE_HEADER if not span else sfd.GLOBAL_ZSCORE_HEADER[:-1] + "\tSpan\n"
    assert open(str(tmp_path / "rec") + ".global_zscore.txt").read() == header + "\t".join(row + ([str(span)] if span else [])) + "\n"

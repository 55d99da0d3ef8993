"""Which entry point and which kernels a whole record reaches ("Routes of the whole-record folds"), without a GPU.

Past SF_MAX_W (400 nt) the library has seven whole-record entry points, and every one of them computes the same values as
its neighbours: a record sent to the wrong one is only slower, or single where it should be batched.  The emulation build
(tests/emul) logs the kernel of every launch; each case below makes ONE Python-level call on a record of 401 nt, the first
length past the window limit, and compares the log, consecutive repeats collapsed, to a literal.  Span 100 is the widest with
4 span <= 401 (banded tables), span 101 the first that stays in full tables.  The long and banded partition functions launch
their inside and outside diagonals through a parameter, which the log spells `kernel`; the exterior kernel after it names the
family.  A constraint adds no launch in either layout: the host parses it and copies its arrays up.  For the two drivers
the Engine calls themselves are
recorded too, with their constraints: the MFE folds run in the order -1, -2, free and the ensembles in the order free, -1, -2.
The first half of this file (15 cases) was written against the code as it stood before scanfold_amd/whole.py owned the
routing and passes there unchanged; the second half checks the router's pure functions at every edge, the pre-flight checks
of scanfold.main, and Engine.saved_model()."""
import re

import numpy as np
import pytest

from scanfold_amd import RNA, _lib, functions, params
from scanfold_amd import scanfold as sfd
from long_util import rand_seq

L = _lib.SF_MAX_W + 1
SEQ = rand_seq(np.random.default_rng(401), L)
SHORT = rand_seq(np.random.default_rng(120), 120)
CONS1 = "." * 10 + "(" + "." * 19 + ")" + "." * (L - 31)  # the -1 line: one bracket pair
CONS2 = "." * 5 + "x" + "." * (L - 6)                      # the -2 line: one base kept unpaired

LONG = ["sf_long_fill_kernel", "sf_long_f5_kernel", "sf_long_trace_kernel"]
BAND = ["sf_band_fill_kernel", "sf_band_f5_kernel", "sf_band_trace_kernel"]
LONGB = ["sf_longb_fill_kernel", "sf_longb_f5_kernel"]
BANDB = ["sf_bandb_fill_kernel", "sf_bandb_f5_kernel"]
WINDOW = ["sf_mfe_fast_kernel", "sf_mfe_full_kernel"]
PF_LONG = ["kernel", "sf_pflong_exterior_kernel", "kernel", "sf_pflong_prob_kernel", "sf_pflong_finish_kernel"]
PF_BAND = ["kernel", "sf_pfband_exterior_kernel", "kernel", "sf_pfband_prob_kernel", "sf_pfband_finish_kernel"]
PF_LONGB = ["sf_pflongb_inside_kernel", "sf_pflongb_exterior_kernel", "sf_pflongb_outside_kernel", "sf_pflongb_prob_kernel",
            "sf_pflongb_finish_kernel"]
HC = []  # a constraint adds no launch: the host parses it
LONG_MFE_X3 = (HC + LONG) * 2 + LONG  # the driver's three folds: -1, -2, free
WHOLE = ("fold_long", "fold_long_batch", "fold_banded", "fold_banded_batch", "pf_long", "pf_long_batch", "pf_banded")


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    eng = emul_engine()
    eng.load_params(params.default_params())
    return eng


@pytest.fixture(autouse=True)
def shared_engine(emul, monkeypatch):
    """The emulation is the process-wide engine; afterwards 37 C and no span, set through the facade so that its record of
    the span stays true."""
    monkeypatch.setattr(_lib, "_engine", emul)
    yield
    RNA._check_md(None)
    assert emul.max_bp_span == 0 and emul.params.temperature == 37.0


def launched(eng, call):
    """-> (what call() returned, the kernel families it launched with consecutive repeats collapsed)"""
    from emul_engine import launch_log
    launch_log(eng)
    out = call()
    log = []
    for name in launch_log(eng):
        family = re.sub(r"\s+", "", name).strip("()").partition("<")[0]
        if not log or log[-1] != family:
            log.append(family)
    return out, log


def recorded(eng, monkeypatch):
    """-> a list that every whole-record Engine call from now on appends (method, constraint argument) to"""
    calls = []
    for name in WHOLE:
        def through(rows, cons=None, *a, _real=getattr(eng, name), _name=name, **kw):
            calls.append((_name, cons))
            return _real(rows, cons, *a, **kw)
        monkeypatch.setattr(eng, name, through)
    return calls


def model_under(span):
    m = RNA.md()
    m.max_bp_span = span
    return m


# ---- one call each: the facade, the functions module, the engine ----

@pytest.mark.parametrize("span,want", [(None, LONG), (100, BAND), (101, LONG)])
def test_facade_mfe(emul, span, want):
    fc = RNA.fold_compound(SEQ, None if span is None else model_under(span))
    assert launched(emul, fc.mfe)[1] == want
    assert emul.max_bp_span == (span or 0)


def test_energies_folds_the_long_rows_in_one_batch(emul):
    assert launched(emul, lambda: functions.energies([SEQ, SHORT, SEQ]))[1] == LONGB + WINDOW


def test_rna_refold(emul, tmp_path):
    (tmp_path / "c.txt").write_text(SEQ + "\n" + CONS1 + "\n")
    assert launched(emul, lambda: functions.rna_refold(SEQ, 37, str(tmp_path / "c.txt")))[1] == HC + LONG + HC + PF_LONG


def test_engine_pf_long_batch(emul):
    assert launched(emul, lambda: emul.pf_long_batch([SEQ] * 3, [None, CONS1, CONS2]))[1] == HC + PF_LONGB


def test_engine_pf_banded(emul):
    emul.set_max_bp_span(60)
    try:
        assert launched(emul, lambda: emul.pf_banded(SEQ))[1] == PF_BAND
    finally:
        emul.set_max_bp_span(0)


def test_engine_fold_banded_batch(emul):
    emul.set_max_bp_span(60)
    try:
        assert launched(emul, lambda: emul.fold_banded_batch([SEQ, SEQ[:-1]]))[1] == BANDB
    finally:
        emul.set_max_bp_span(0)


# ---- the two drivers, called directly on the record and three dbn files ----

@pytest.fixture()
def dbn_files(tmp_path):
    base = str(tmp_path / "rec")
    for tag, line in (("no_filter", "." * L), ("-1", CONS1), ("-2", CONS2)):
        with open(base + ".ScanFold." + tag + ".dbn", "w") as w:
            w.write(">rec\n" + SEQ + "\n" + line + "\n")
    return base


MFE_ORDER = [CONS1, CONS2, None]
ENS_ORDER = [None, CONS1, CONS2]


@pytest.mark.parametrize("case,kw,calls,kernels", [
    ("span=0", dict(), [("fold_long", c) for c in MFE_ORDER], LONG_MFE_X3),
    ("span=60", dict(span=60), [("fold_banded", c) for c in MFE_ORDER], BAND * 3),
    ("ensemble", dict(ensemble=True), [("fold_long", c) for c in MFE_ORDER] + [("pf_long_batch", ENS_ORDER)],
     LONG_MFE_X3 + HC + PF_LONGB),
    ("ensemble, no batch", dict(ensemble=True), [("fold_long", c) for c in MFE_ORDER] + [("pf_long", c) for c in ENS_ORDER],
     LONG_MFE_X3 + PF_LONG + (HC + PF_LONG) * 2),
    ("ensemble_banded", dict(span=60, ensemble_banded=True),
     [("fold_banded", c) for c in MFE_ORDER] + [("pf_banded", c) for c in ENS_ORDER], BAND * 3 + PF_BAND * 3),
])
def test_global_refold(emul, monkeypatch, dbn_files, case, kw, calls, kernels):
    if case == "ensemble, no batch":
        monkeypatch.setattr(emul, "has_pf_long_batch", lambda: False)
    got = recorded(emul, monkeypatch)
    params0 = emul.params
    _, log = launched(emul, lambda: sfd.global_refold(SEQ, "rec", dbn_files, 37, **kw))
    assert got == calls
    assert log == kernels
    assert emul.params is params0 and emul.max_bp_span == 0


@pytest.mark.parametrize("span,call,kernels", [(0, "fold_long_batch", LONGB), (60, "fold_banded_batch", BANDB)])
def test_global_zscore(emul, monkeypatch, tmp_path, span, call, kernels):
    got = recorded(emul, monkeypatch)
    params0 = emul.params
    _, log = launched(emul, lambda: sfd.global_zscore(SEQ, "rec", str(tmp_path / "rec"), 37, 2, "mono", seed=3, span=span))
    assert got == [(call, None)]
    assert log == kernels
    assert emul.params is params0 and emul.max_bp_span == 0


# ---- the router's pure functions, at every edge, without an engine ----

from scanfold_amd import whole  # noqa: E402

W, LONGEST, BANDED = _lib.SF_MAX_W, _lib.SF_MAX_LONG, _lib.SF_MAX_BANDED
ALL = frozenset(whole.ENTRY_POINTS)


def test_the_limits_are_the_headers():
    assert (W, LONGEST, BANDED) == (400, 32767, 4194304)


@pytest.mark.parametrize("n,span,want", [
    (W, 0, ("window", W)), (W, 100, ("window", W)),
    (W + 1, 0, ("fold_long", LONGEST)), (W + 1, 100, ("fold_banded", BANDED)), (W + 1, 101, ("fold_long", LONGEST)),
    (404, 101, ("fold_banded", BANDED)),   # 4 span = L
    (403, 101, ("fold_long", LONGEST)),    # 4 span = L + 1
    (LONGEST, 0, ("fold_long", LONGEST)), (LONGEST, 8192, ("fold_long", LONGEST)), (LONGEST, 8191, ("fold_banded", BANDED)),
    (LONGEST + 1, 1, ("fold_banded", BANDED)), (LONGEST + 1, LONGEST, ("fold_banded", BANDED)),  # (no room left in full tables)
    (BANDED, 600, ("fold_banded", BANDED)), (BANDED + 1, 600, ("fold_banded", BANDED)),  # (past its limit: the library refuses)
])
def test_mfe_route_auto(n, span, want):
    assert whole.mfe_route(n, span, False, whole.AUTO, ALL) == want
    many = (want[0] if want[0] == "window" else want[0] + "_batch", want[1])
    assert whole.mfe_route(n, span, True, whole.AUTO, ALL) == many


def test_mfe_route_auto_refusals():
    for n in (LONGEST + 1, BANDED, BANDED + 1):
        with pytest.raises(ValueError, match="max_bp_span"):
            whole.mfe_route(n, 0, False, whole.AUTO, ALL)
    with pytest.raises(NotImplementedError, match="SHAPE"):
        whole.mfe_route(W + 1, 0, False, whole.AUTO, ALL, shape=True)
    with pytest.raises(NotImplementedError, match="SHAPE"):  # before the length is looked at
        whole.mfe_route(LONGEST + 1, 0, False, whole.AUTO, ALL, shape=True)
    assert whole.mfe_route(W, 0, False, whole.AUTO, ALL, shape=True) == ("window", W)


def test_mfe_route_without_the_banded_entry_point():
    some = ALL - {"fold_banded", "fold_banded_batch"}
    assert whole.mfe_route(W + 1, 100, False, whole.AUTO, some) == ("fold_long", LONGEST)
    assert whole.mfe_route(W + 1, 100, True, whole.AUTO, some) == ("fold_long_batch", LONGEST)
    # past the full tables there is nowhere else to go: the Engine call names the missing symbol
    assert whole.mfe_route(LONGEST + 1, 100, False, whole.AUTO, some) == ("fold_banded", BANDED)
    # a flag that asks for banded tables gets them, or the Engine call's error
    assert whole.mfe_route(W + 1, 100, False, whole.ALWAYS, some) == ("fold_banded", BANDED)


@pytest.mark.parametrize("n", [1, W, W + 1, LONGEST, LONGEST + 1, BANDED, BANDED + 1])
@pytest.mark.parametrize("span", [0, 100])
def test_mfe_route_always_and_never(n, span):
    assert whole.mfe_route(n, span, False, whole.ALWAYS, ALL) == ("fold_banded", BANDED)
    assert whole.mfe_route(n, span, True, whole.ALWAYS, ALL) == ("fold_banded_batch", BANDED)
    if n <= W:
        assert whole.mfe_route(n, span, False, whole.NEVER, ALL) == whole.mfe_route(n, span, True, whole.NEVER, ALL) == ("window", W)
    else:  # whatever span is resident, and past the limit too: the library refuses such a row
        assert whole.mfe_route(n, span, False, whole.NEVER, ALL) == ("fold_long", LONGEST)
        assert whole.mfe_route(n, span, True, whole.NEVER, ALL) == ("fold_long_batch", LONGEST)


def test_mfe_route_without_the_batch_entry_point():
    some = ALL - {"fold_long_batch"}
    with pytest.raises(_lib.ScanFoldHipError, match=r"sf_fold_long_batch, which this library \(libx\.so\) does not export"):
        whole.mfe_route(W + 1, 0, True, whole.NEVER, some, library="libx.so")
    assert whole.mfe_route(W, 0, True, whole.NEVER, some) == ("window", W)
    assert whole.mfe_route(W + 1, 0, False, whole.NEVER, some) == ("fold_long", LONGEST)


@pytest.mark.parametrize("n", [1, W, W + 1, LONGEST, LONGEST + 1, BANDED, BANDED + 1])
def test_pf_route(n):
    for span in (0, 100):
        if n <= W:
            for policy in (whole.AUTO, whole.NEVER):
                assert whole.pf_route(n, span, False, policy, ALL) == whole.pf_route(n, span, True, policy, ALL) == ("window", W)
        else:
            with pytest.raises(NotImplementedError, match="no partition function"):
                whole.pf_route(n, span, False, whole.AUTO, ALL)
            assert whole.pf_route(n, span, False, whole.NEVER, ALL) == ("pf_long", LONGEST)
            assert whole.pf_route(n, span, True, whole.NEVER, ALL) == ("pf_long_batch", LONGEST)
            assert whole.pf_route(n, span, True, whole.NEVER, ALL - {"pf_long_batch"}) == ("pf_long", LONGEST)
    for many in (False, True):  # there is no banded batch
        assert whole.pf_route(n, 100, many, whole.ALWAYS, ALL) == ("pf_banded", BANDED)
        assert whole.pf_route(n, 100, many, whole.ALWAYS, ALL - {"pf_banded"}) == ("pf_banded", BANDED)
        with pytest.raises(ValueError, match="the banded ensemble needs a base-pair span"):
            whole.pf_route(n, 0, many, whole.ALWAYS, ALL)


def test_exports_follow_the_engine(emul, monkeypatch):
    assert whole.exports(emul) == ALL
    monkeypatch.setattr(emul, "has_pf_long_batch", lambda: False)
    assert whole.exports(emul) == ALL - {"pf_long_batch"}


def test_preflight_reads_the_fasta_file_at_most_once(tmp_path, monkeypatch):
    """Three checks look at the records' lengths (--global_span with --global_zscore, --global_ensemble_banded,
    --global_zscore): one read.  A run none of whose flags has a limit reads nothing before the engine is asked for.  The
    limits in the messages are the router's."""
    from scanfold_amd import scan as scanmod

    class Reached(Exception):
        pass

    def no_engine(device=None):
        raise Reached()

    monkeypatch.chdir(tmp_path)
    (tmp_path / "in.fa").write_text(">ok\nACGU\n>big\n" + "A" * LONGEST + "\n")
    reads = []
    real = scanmod.read_fasta
    with monkeypatch.context() as m:  # (undone before the module's fixture asks for the engine again)
        m.setattr(scanmod, "read_fasta", lambda path: (reads.append(path), real(path))[1])
        m.setattr(_lib, "get_engine", no_engine)
        with pytest.raises(Reached):
            sfd.main(["in.fa", "--global_refold", "--global_span", "50", "--global_ensemble_banded", "--global_zscore"])
        assert reads == ["in.fa"]
        del reads[:]
        with pytest.raises(Reached):
            sfd.main(["in.fa", "--global_refold", "--global_span", "50"])
        assert reads == []
        (tmp_path / "in.fa").write_text(">ok\nACGU\n>big\n" + "A" * (LONGEST + 1) + "\n")
        with pytest.raises(ValueError, match="--global_zscore: record big has %d nt, whole-record folds stop at %d" % (LONGEST + 1, LONGEST)):
            sfd.main(["in.fa", "--global_zscore"])
        with pytest.raises(ValueError, match=r"--global_span: record big has %d nt; --global_ensemble \(.*\) stops at %d nt"
                           % (LONGEST + 1, LONGEST)):
            sfd.main(["in.fa", "--global_refold", "--global_span", "50", "--global_ensemble"])
        with pytest.raises(Reached):  # banded tables take it
            sfd.main(["in.fa", "--global_refold", "--global_span", "50", "--global_ensemble_banded", "--global_zscore_span", "60"])


# ---- Engine.saved_model() ----

@pytest.fixture()
def par_engine(emul):
    """the emulation with a parameter set that has enthalpies, so that the temperature can change"""
    from par_util import par_text, synthetic_enthalpies
    base = params.default_params()
    emul.load_params(params.parse_par_text(par_text(base.rec, synthetic_enthalpies(base.rec, 5)), source="synthetic.par"))
    yield emul
    emul.load_params(params.default_params())


def loads_counted(eng, monkeypatch):
    loads = []
    real = eng._load
    monkeypatch.setattr(eng, "_load", lambda p: (loads.append(p), real(p))[1])
    return loads


@pytest.mark.parametrize("raises", [False, True])
def test_saved_model_restores_temperature_span_and_md_span(par_engine, monkeypatch, raises):
    eng = par_engine
    eng.set_max_bp_span(25)
    eng.md_span = 7
    params0 = eng.params
    loads = loads_counted(eng, monkeypatch)
    try:
        with eng.saved_model() as scope:
            assert scope is eng
            eng.set_temperature(50)
            eng.set_max_bp_span(60)
            eng.md_span = 60
            assert eng.params is not params0 and eng.params.temperature == 50.0 and loads == [eng.params]
            if raises:
                raise KeyError("a fold failed")
    except KeyError:
        assert raises
    try:
        assert eng.params is params0 and loads[1:] == [params0]  # uploaded again, once
        assert (eng.max_bp_span, eng.md_span) == (25, 7)
    finally:
        eng.set_max_bp_span(0)
        eng.md_span = 0


def test_a_scope_in_which_nothing_changed_uploads_nothing(emul, monkeypatch):
    loads = loads_counted(emul, monkeypatch)
    with emul.saved_model():
        emul.set_temperature(37)  # (already resident)
        emul.fold_long("ACGU" * 5)
    assert loads == []
    assert (emul.max_bp_span, emul.md_span) == (0, 0)


def test_scopes_nest(par_engine):
    eng = par_engine
    params0 = eng.params
    with eng.saved_model():
        eng.set_max_bp_span(30)
        eng.set_temperature(45)
        p1 = eng.params
        with eng.saved_model():
            eng.set_max_bp_span(0)
            eng.md_span = 9
            eng.set_temperature(60)
        assert (eng.max_bp_span, eng.md_span) == (30, 0) and eng.params is p1
    assert (eng.max_bp_span, eng.md_span) == (0, 0) and eng.params is params0


def test_the_facade_records_the_span_it_made_resident(emul):
    """Engine.md_span is declared (0), follows the facade, and a model without a span leaves a span set beside the facade
    alone: what keeps the scan's --span through the motif refolds."""
    assert emul.md_span == 0
    emul.set_max_bp_span(25)
    try:
        RNA.fold_compound("ACGU" * 5).mfe()
        assert (emul.max_bp_span, emul.md_span) == (25, 0)
        RNA.fold_compound("ACGU" * 5, model_under(40)).mfe()
        assert (emul.max_bp_span, emul.md_span) == (40, 40)
    finally:
        RNA._check_md(None)
    assert (emul.max_bp_span, emul.md_span) == (0, 0)

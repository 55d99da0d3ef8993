"""Which kernel a batch of windows runs on ("Routes of the windowed folds"), without a GPU.

Every other test compares values, and every route computes the same values: a batch sent to the wrong kernel is only slower
(the constrained partition function above 120 nt ran ~90 x slower for four rounds that way).  The emulation build
(tests/emul) logs the kernel of every launch as its call site spells it; one fold per case, and the log must be the literal
below — the route table of the host file as it stood before launch_pf / launch_mfe owned the routing, which this test passed
on unchanged.  For the partition-function kernels the template arguments count too: sf_pf_lds_kernel<WT, SH, HC> and
sf_pf_fast_kernel<NT, WT, HC>, a trailing argument left to its default (false) written out."""
import re

import numpy as np
import pytest

from scanfold_amd import _lib, params

GEN, REDO = "sf_pf_kernel<false>", "sf_pf_kernel<true>"
FULL, FAST = "sf_mfe_full_kernel", "sf_mfe_fast_kernel"
WIDTHS = (15, 16, 120, 121, 250, 251, 256, 257)

# kernel mode 0, by width: the plain folds, the folds under a constraint whose bracket pairs can pair, and the MFE kernels
PF_PLAIN = {15: GEN, 16: "sf_pf_lds_kernel<0,false,false>", 120: "sf_pf_lds_kernel<120,false,false>",
            121: "sf_pf_fast_kernel<128,0,false>", 250: "sf_pf_fast_kernel<256,0,false>",
            251: "sf_pf_fast_kernel<256,0,false>", 256: "sf_pf_fast_kernel<256,0,false>", 257: GEN}
PF_CONS = {15: GEN, 16: "sf_pf_lds_kernel<0,false,true>", 120: "sf_pf_lds_kernel<0,false,true>",
           121: "sf_pf_fast_kernel<128,0,true>", 250: "sf_pf_fast_kernel<256,0,true>", 251: GEN, 256: GEN, 257: GEN}
MFE_PLAIN = {15: [FULL], 16: [FAST, FULL], 120: [FAST, FULL], 121: [FAST, FULL], 250: [FAST, FULL], 251: [FAST, FULL],
             256: [FAST, FULL], 257: [FULL]}
MFE_CONS = {15: [FULL], 16: [FAST, FULL], 120: [FAST, FULL], 121: [FAST, FULL], 250: [FAST, FULL], 251: [FULL],
            256: [FULL], 257: [FULL]}

_DEFAULTS = {"sf_pf_lds_kernel": 3, "sf_pf_fast_kernel": 3}  # template arguments; the ones left out default to false


def spelled(name):
    """'(sf_pf_lds_kernel<120, true>)' -> 'sf_pf_lds_kernel<120,true,false>'; an MFE or shuffle kernel -> its family"""
    s = re.sub(r"\s+", "", name).strip("()")
    family, _, rest = s.partition("<")
    if not family.startswith("sf_pf_"):
        return family
    args = rest.rstrip(">").split(",")
    args += ["false"] * (_DEFAULTS.get(family, len(args)) - len(args))
    return "%s<%s>" % (family, ",".join(args))


@pytest.fixture(scope="module")
def emul():
    from emul_engine import emul_engine
    eng = emul_engine()
    yield eng
    eng.set_kernel_mode(0)
    eng.load_params(params.default_params())


def launched(eng, call):
    from emul_engine import launch_log
    launch_log(eng)
    call()
    return [spelled(k) for k in launch_log(eng)]


def window(W, kind):
    """One fold of the cheapest sequence: no base can pair but the two ends, G and C (a type-7 pair: A and A)."""
    if kind == "type7":
        return ["A" * W], ["(" + "." * (W - 2) + ")"]
    return ["G" + "A" * (W - 2) + "C"], (None if kind == "plain" else ["(" + "." * (W - 2) + ")"])


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("kind", ["plain", "cons", "type7"])
def test_fold_routes(emul, W, kind):
    emul.load_params(params.default_params())
    seqs, cons = window(W, kind)
    for mode in (0, 1):
        emul.set_kernel_mode(mode)
        try:
            got = launched(emul, lambda: emul.fold_constrained(seqs, cons))
        finally:
            emul.set_kernel_mode(0)
        if mode == 1 or kind == "type7":
            want = [FULL, GEN, REDO]
        else:
            want = (MFE_PLAIN if kind == "plain" else MFE_CONS)[W] + [(PF_PLAIN if kind == "plain" else PF_CONS)[W], REDO]
        assert got == want, (W, kind, mode)


@pytest.mark.parametrize("W", WIDTHS)
def test_pf_batch_routes(emul, W):
    emul.load_params(params.default_params())
    seqs, _ = window(W, "plain")
    assert launched(emul, lambda: emul.pf_batch(seqs)) == [PF_PLAIN[W], REDO]
    emul.set_kernel_mode(1)
    try:
        assert launched(emul, lambda: emul.pf_batch(seqs)) == [GEN, REDO]
    finally:
        emul.set_kernel_mode(0)


def test_shape_data_alone_are_a_plain_partition_function(emul):
    """Deigan pseudo-energies without a constraint row: the MFE kernel's constrained instantiation (same family), the
    plain partition-function kernel with the width folded in."""
    emul.load_params(params.default_params())
    seqs, _ = window(120, "plain")
    sc = np.full((1, 120), -20, dtype=np.int32)
    assert launched(emul, lambda: emul.fold_constrained(seqs, None, sc)) == [FAST, FULL, "sf_pf_lds_kernel<120,false,false>", REDO]


@pytest.mark.parametrize("step,pf", [(1, "sf_pf_lds_kernel<120,true,false>"), (40, "sf_pf_lds_kernel<120,false,false>")])
def test_scan_routes(emul, step, pf):
    """sf_scan at W = 120 over three windows (no shuffles): step 1 shares the inside pass (SH), step 40 (> W / 4) does not."""
    emul.load_params(params.default_params())
    tr = "G" + "A" * (118 + 2 * step) + "C"
    got = launched(emul, lambda: emul.scan(tr, 120, step, 0, 3, 0, _lib.SHUFFLE_MONO, 3))
    assert got == ["sf_shuffle_kernel", FAST, FULL, pf, REDO]


@pytest.mark.parametrize("W", [16, 120, 256])
def test_mfe_without_the_int16_kernel(emul, W):
    """A parameter set with an entry past SF_FAST_MAXPARAM (fast_ok = 0): the MFE goes to the general kernel at every width,
    the partition function's route does not depend on it."""
    from par_util import SF_FAST_MAXPARAM, boundary_params
    emul.load_params(boundary_params(3, SF_FAST_MAXPARAM + 1))
    try:
        seqs, cons = window(W, "cons")
        assert launched(emul, lambda: emul.mfe_batch(seqs)) == [FULL]
        assert launched(emul, lambda: emul.fold_constrained(seqs, cons)) == [FULL, PF_CONS[W], REDO]
        emul.load_params(boundary_params(3))  # the same set within the bound: the int16 kernel again
        assert launched(emul, lambda: emul.mfe_batch(seqs)) == [FAST, FULL]
    finally:
        emul.load_params(params.default_params())

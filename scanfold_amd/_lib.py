"""ctypes binding of libscanfold_hip.so (include/scanfold_hip.h) — the only compute path of this package.

There is no CPU fallback: if the shared library is missing or no GPU is usable, `get_engine()` raises.
(The reference's compute path is ViennaRNA on the CPU through a 12-process pool,
ScanFold-Scan.py:73-77,244-262; nothing of it is kept.)
"""
import contextlib
import ctypes
import os

import numpy as np

from . import params as _params

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libscanfold_hip.so")

SHUFFLE_MONO = 0
SHUFFLE_DI = 1
SCAN_NO_PF = 1
SCAN_NO_TRACE = 2

_c_u8p = ctypes.c_void_p
_EXPORTS = {
    "sf_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "sf_last_hip_error": (ctypes.c_char_p, []),
    "sf_init": (ctypes.c_int, [ctypes.c_int]),
    "sf_shutdown": (ctypes.c_int, []),
    "sf_device_name": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "sf_params_load": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double]),
    "sf_params_load_rescaled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_char_p,
                                               ctypes.c_char_p]),
    "sf_mfe_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "sf_mfe_batch_dev": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_mfe_trace_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_pf_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p]),
    "sf_fold_constrained": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_shuffle_windows": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.c_void_p]),
    "sf_scan": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_scan_dev": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p]),
    "sf_tabulate_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_int64)]),
    "sf_tabulate_fetch": (ctypes.c_int, [ctypes.c_void_p] * 7),
    "sf_last_status": (ctypes.c_int, []),
    "sf_prof_stop": (ctypes.c_int, []),
    "sf_set_kernel_mode": (ctypes.c_int, [ctypes.c_int]),
    "sf_set_max_bp_span": (ctypes.c_int, [ctypes.c_int]),
    "sf_prof_reset": (ctypes.c_int, []),
    "sf_prof_get": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int64)]),
}
EXPORTED_SYMBOLS = tuple(_EXPORTS)



def _header_define(header, name):
    """the integer value of `#define name` in include/<header>: the library's limits, read from the header it is compiled from"""
    import re
    path = os.path.join(os.path.dirname(_HERE), "include", header)
    with open(path) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, f.read(), flags=re.M)
    if m is None:
        raise ScanFoldHipError("%s defines no %s" % (path, name))
    return int(m.group(1))


# include/scanfold_hip_long.h: bound only where the loaded library exports them (the CPU twin of the C ABI does not)
_LONG_EXPORTS = {
    "sf_fold_long": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_fold_long_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 3),
    "sf_fold_banded": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]),
    "sf_fold_banded_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2),
    "sf_fold_banded_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "sf_fold_long_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "sf_fold_long_batch_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(ctypes.c_int)]),
    "sf_set_long_batch_bytes": (ctypes.c_int, [ctypes.c_size_t]),
    "sf_fold_banded_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "sf_fold_banded_batch_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2),
    "sf_pf_long": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p]),
    "sf_pf_long_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]),
    "sf_pf_banded": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "sf_pf_banded_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 2 + [ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_int)] * 2),
    "sf_pf_banded_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "sf_pf_banded_probs": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_double]
                           + [ctypes.c_void_p] * 6 + [ctypes.POINTER(ctypes.c_size_t)]),
    "sf_pf_probs_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "sf_pf_banded_probs_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_size_t),
                                                ctypes.POINTER(ctypes.c_size_t)]),
    "sf_mea_pairs": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_double,
                                    ctypes.c_void_p, ctypes.c_void_p]),
    "sf_pf_banded_mea": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
                         + [ctypes.c_void_p] * 6 + [ctypes.POINTER(ctypes.c_size_t)] + [ctypes.c_void_p] * 2),
    "sf_mea_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2
                     + [ctypes.POINTER(ctypes.c_size_t)]),
    "sf_pf_long_batch": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5),
    "sf_pf_long_batch_times": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
}
# one row of sf_pf_long_batch (struct sf_pf_long_row) and its "no hint for this row" (SF_PF_LONG_NO_HINT)
PF_LONG_ROW_DTYPE = np.dtype([("ens_dG", np.float64), ("mean_bp_dist", np.float64), ("centroid_dist", np.float64),
                              ("lns", np.float64), ("attempts", np.int32), ("reserved", np.int32)])
SF_PF_LONG_NO_HINT = -2 ** 31
# one listed base pair of sf_pf_banded_probs (struct sf_pair_prob): 1-based positions, i < j
PAIR_PROB_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("p", "<f8")])


# include/scanfold_hip_duplex.h: likewise optional (duplex folds and the LRI scan)
_DUPLEX_EXPORTS = {
    "sf_duplex_batch": (ctypes.c_int, [_c_u8p, _c_u8p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6),
    "sf_lri_grid": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(ctypes.c_int32)]),
    "sf_lri_scan": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p]),
    "sf_lri_scan_time": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "sf_lri_background": (ctypes.c_int, [_c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
}
# one compacted hit of sf_lri_scan (struct sf_lri_hit)
LRI_HIT_DTYPE = np.dtype([("j_win", np.int32), ("k_win", np.int32), ("energy", np.int32), ("i", np.int32),
                          ("j", np.int32)])


def _header_value(header, name):
    """like _header_define for a `#define name` whose value is signed or a parenthesised integer expression"""
    import re
    path = os.path.join(os.path.dirname(_HERE), "include", header)
    with open(path) as f:
        m = re.search(r"^#define\s+%s\s+([-+0-9() ]+?)\s*(?:/\*|$)" % name, f.read(), flags=re.M)
    if m is None:
        raise ScanFoldHipError("%s defines no integer %s" % (path, name))
    return int(eval(m.group(1), {"__builtins__": {}}))


class ScanFoldHipError(RuntimeError):
    pass


SF_MAX_W = _header_define("scanfold_hip.h", "SF_MAX_W")  # longest window of the window kernels
SF_MAX_LONG = _header_define("scanfold_hip_long.h", "SF_MAX_LONG")  # longest sequence of sf_fold_long
SF_MAX_BANDED = _header_define("scanfold_hip_long.h", "SF_MAX_BANDED")  # longest sequence of sf_fold_banded
SF_DUPLEX_MAX_LEN = _header_define("scanfold_hip_duplex.h", "SF_DUPLEX_MAX_LEN")  # longest strand of a duplex
SF_DUPLEX_STRUCT_LEN = _header_define("scanfold_hip_duplex.h", "SF_DUPLEX_STRUCT_LEN")
SF_DUPLEX_NONE = _header_define("scanfold_hip_duplex.h", "SF_DUPLEX_NONE")  # "energy" of strands that cannot pair
SF_DUPLEX_SKIPPED = _header_value("scanfold_hip_duplex.h", "SF_DUPLEX_SKIPPED")  # dense scan: left out by the distance test
SF_ERR_DUPLEX_HITS = _header_value("scanfold_hip_duplex.h", "SF_ERR_DUPLEX_HITS")

# Engine._need's arguments: an entry point only libscanfold_hip.so exports, and what needs it
_FOLD_LONG = ("sf_fold_long", "whole-record folds")
_FOLD_BANDED = ("sf_fold_banded", "whole-record folds under a base-pair span in banded tables")
_FOLD_LONG_BATCH = ("sf_fold_long_batch", "folds of sequences past %d nt" % SF_MAX_W)
_FOLD_BANDED_BATCH = ("sf_fold_banded_batch", "batched whole-record folds under a base-pair span in banded tables")
_PF_LONG = ("sf_pf_long", "whole-record partition functions")
_PF_BANDED = ("sf_pf_banded", "whole-record partition functions under a base-pair span in banded tables")
_PF_BANDED_PROBS = ("sf_pf_banded_probs", "base-pair probabilities of a whole record under a base-pair span")
_MEA_PAIRS = ("sf_mea_pairs", "maximum-expected-accuracy structures of a pair list")
_PF_BANDED_MEA = ("sf_pf_banded_mea", "maximum-expected-accuracy structures of a whole record under a base-pair span")
_PF_LONG_BATCH = ("sf_pf_long_batch", "partition functions of many sequences past %d nt" % SF_MAX_W)
_DUPLEX = ("duplex entry points (sf_duplex_batch, sf_lri_scan, sf_lri_background)", "duplex folds and --lri",
           tuple(_DUPLEX_EXPORTS))
_D, _I, _Z = ctypes.c_double, ctypes.c_int, ctypes.c_size_t  # Engine._times' field types


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64 (same SONAME, different file name).  Two HIP runtimes in
    one process do not work ("No HIP GPUs are available" in whichever initialises second), so when torch is
    installed its copy is loaded first and this library binds to it by SONAME; torch later finds the same
    file already loaded.  Without torch the system runtime under /opt/rocm is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path=LIB_PATH):
    """dlopen the C-ABI library and declare every prototype; raises if it or a symbol is missing."""
    if not os.path.exists(path):
        raise ScanFoldHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    if os.path.abspath(path) == os.path.abspath(LIB_PATH):
        _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(path)
    for name, (res, args) in _EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in list(_LONG_EXPORTS.items()) + list(_DUPLEX_EXPORTS.items()):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return lib


def seqs_to_array(seqs, W=None):
    """list of equal-length str / bytes, or a uint8 (n, W) array -> contiguous uint8 (n, W)."""
    if isinstance(seqs, np.ndarray):
        arr = np.ascontiguousarray(seqs, dtype=np.uint8)
        if arr.ndim != 2:
            raise ValueError("sequence array must be 2-D (n, W)")
        return arr
    seqs = [_ascii(s) for s in seqs]
    if not seqs:
        return np.zeros((0, W or 1), dtype=np.uint8)
    W = len(seqs[0])
    if any(len(s) != W for s in seqs):
        raise ValueError("all sequences of one batch must have the same length")
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), W)


def _ascii(s):
    """str, bytes or bytearray -> the bytes the C ABI reads"""
    return s if isinstance(s, (bytes, bytearray)) else str(s).encode("ascii")


def _record(seq, cons):
    """one sequence and its constraint string or None -> (uint8 array, L, constraint bytes or None)"""
    s = _ascii(seq)
    L = len(s)
    c = None if cons is None else bytes(_ascii(cons))
    if c is not None and len(c) != L:
        raise ValueError("constraint string and sequence differ in length")
    return (np.frombuffer(bytes(s), dtype=np.uint8) if L else np.zeros(1, dtype=np.uint8)), L, c


def _pad(rows, ld, fill=0):
    """byte strings of any lengths (None: an empty one) -> uint8 (n, ld), every row filled up with `fill`"""
    arr = np.full((len(rows), ld), fill, dtype=np.uint8)
    for k, s in enumerate(rows):
        if s:
            arr[k, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return arr


def _ragged_rows(seqs, cons=None):
    """sequences of any lengths and None or one constraint item per sequence (a string of its length, or None) ->
    (uint8 (n, ld), int32 lengths, ld, uint8 (n, ld) of constraint rows filled up with dots, or None where no row has one)"""
    rows = [_ascii(s) for s in seqs]
    ld = max([1] + [len(s) for s in rows])
    c = None
    if cons is not None:
        cons = [None if x is None else _ascii(x) for x in cons]
        if len(cons) != len(rows):
            raise ValueError("one constraint item (a string or None) per sequence")
        if any(x is not None and len(x) != len(s) for x, s in zip(cons, rows)):
            raise ValueError("constraint string and sequence differ in length")
        if any(x is not None for x in cons):
            c = _pad(cons, ld, ord("."))
    return _pad(rows, ld), np.array([len(s) for s in rows], dtype=np.int32), ld, c


class Engine:
    """One process, one GPU.  Thin, stateful wrapper over the C ABI."""

    def __init__(self, device=0, paramset=None, lib_path=LIB_PATH):
        self.lib = load_library(lib_path)
        self._check(self.lib.sf_init(int(device)))
        self.device = int(device)
        self.params = None
        self.max_bp_span = 0  # what the last set_max_bp_span made resident (sf_init: no limit)
        self.md_span = 0  # the span the RNA facade last made resident (RNA._check_md sets it only when a model's differs)
        self.load_params(paramset if paramset is not None else _params.default_params())

    # -- plumbing --
    def _check(self, rc):
        if rc != 0:
            msg = self.lib.sf_strerror(rc).decode()
            if rc == -6:
                msg += ": " + self.lib.sf_last_hip_error().decode()
            raise ScanFoldHipError(msg)

    def _need(self, symbol, what, names=None):
        """Raises ScanFoldHipError on a library without the entry point `symbol` (or without one of `names`, where `symbol`
        describes several), which `what` need: there is no fallback."""
        if any(getattr(self.lib, name, None) is None for name in names or (symbol,)):
            raise ScanFoldHipError("this library (%s) has no %s: %s need libscanfold_hip.so"
                                   % (getattr(self.lib, "_name", "?"), symbol, what))

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.sf_device_name(buf, 256))
        return buf.value.decode()

    def load_params(self, paramset, temperature=None):
        """RNA.md() + RNA.fold_compound(seq, md): make `paramset` the folding model.  `temperature` other than the
        set's own rescales it first (ParamSet.at_temperature: needs the enthalpy tables of a real .par file)."""
        if temperature is not None and float(temperature) != paramset.temperature:
            paramset = paramset.at_temperature(temperature)
        self._load(paramset)
        self.params = paramset
        self._by_temp = {paramset.temperature: paramset}

    def _load(self, p):
        blob = p.blob()
        b37, bdh = p.rescale_blobs()
        self._check(self.lib.sf_params_load_rescaled(blob, len(blob), p.temperature, b37, bdh))

    def set_temperature(self, temperature):
        """md.temperature = T (ScanFold-Scan.py:70-71; ScanFoldFunctions.py:776-777): switch the resident model to the
        loaded set rescaled to T; a no-op when it is already there.  Raises NotImplementedError for a set without
        enthalpies (the reconstructed default) when T is not the set's temperature."""
        t = float(temperature)
        if t == self.params.temperature:
            return
        cache = self._by_temp
        if t not in cache:
            cache[t] = self.params.at_temperature(t)
        p = cache[t]
        self._load(p)
        self.params = p

    @contextlib.contextmanager
    def saved_model(self):
        """A scope around folds under another model: on exit, also on an exception, the parameter set (and so the temperature),
        the base-pair span and the facade's record of it are as they were on entry.  The set is uploaded again only where
        the scope left another one resident."""
        params0, span0, md_span0 = self.params, self.max_bp_span, self.md_span
        try:
            yield self
        finally:
            if self.params is not params0:
                self._load(params0)
                self.params = params0
            self.set_max_bp_span(span0)
            self.md_span = md_span0

    def _times(self, need, **fields):
        """the out-parameters of <entry point>_times, `fields` naming them in the C order with their types -> dict"""
        self._need(*need)
        vals = [t() for t in fields.values()]
        self._check(getattr(self.lib, need[0] + "_times")(*(ctypes.byref(v) for v in vals)))
        return {k: v.value for k, v in zip(fields, vals)}

    def shutdown(self):
        self._check(self.lib.sf_shutdown())

    # -- host-buffer entry points --
    def mfe_batch(self, seqs):
        arr = seqs_to_array(seqs)
        n, W = arr.shape
        out = np.empty(n, dtype=np.int32)
        self._check(self.lib.sf_mfe_batch(arr.ctypes.data, n, W, out.ctypes.data))
        return out

    def mfe_trace_batch(self, seqs):
        arr = seqs_to_array(seqs)
        n, W = arr.shape
        out = np.empty(n, dtype=np.int32)
        db = np.zeros((n, W + 1), dtype=np.uint8)
        self._check(self.lib.sf_mfe_trace_batch(arr.ctypes.data, n, W, out.ctypes.data, db.ctypes.data))
        return out, [bytes(row[:W]).decode() for row in db]

    def pf_batch(self, seqs):
        arr = seqs_to_array(seqs)
        n, W = arr.shape
        dG = np.empty(n)
        mbd = np.empty(n)
        cd = np.empty(n)
        cen = np.zeros((n, W + 1), dtype=np.uint8)
        self._check(self.lib.sf_pf_batch(arr.ctypes.data, n, W, dG.ctypes.data, mbd.ctypes.data, cen.ctypes.data,
                                         cd.ctypes.data))
        return dict(dG=dG, mean_bp_dist=mbd, centroid=[bytes(r[:W]).decode() for r in cen], centroid_dist=cd)

    def fold_constrained(self, seqs, cons=None, sc_stack_dcal=None, mfe=True, pf=True):
        """fc.hc_add_from_db / fc.sc_add_SHAPE_deigan + fc.mfe() / fc.pf() on n windows (ScanFold-Scan.py:405-418;
        ScanFold.py:508-544).  cons: list of W-char str or uint8 (n, W); sc_stack_dcal: int32 (n, W).
        -> dict(mfe, structure [str], dG, mean_bp_dist, centroid [str], centroid_dist) (the keys that were asked for)"""
        arr = seqs_to_array(seqs)
        n, W = arr.shape
        c = None if cons is None else seqs_to_array(cons)
        if c is not None and c.shape != (n, W):
            raise ValueError("constraint rows must match the sequence rows")
        s = None if sc_stack_dcal is None else np.ascontiguousarray(sc_stack_dcal, dtype=np.int32).reshape(n, W)
        e = np.zeros(n, dtype=np.int32)
        db = np.zeros((n, W + 1), dtype=np.uint8)
        dG, mbd, cd = np.zeros(n), np.zeros(n), np.zeros(n)
        cen = np.zeros((n, W + 1), dtype=np.uint8)
        flags = (0 if pf else 1) | (0 if mfe else 2)
        self._check(self.lib.sf_fold_constrained(arr.ctypes.data, n, W, None if c is None else c.ctypes.data,
                                                 None if s is None else s.ctypes.data, flags, e.ctypes.data,
                                                 db.ctypes.data, dG.ctypes.data, mbd.ctypes.data, cen.ctypes.data,
                                                 cd.ctypes.data))
        out = {}
        if mfe:
            out.update(mfe=e, structure=[bytes(r[:W]).decode() for r in db])
        if pf:
            out.update(dG=dG, mean_bp_dist=mbd, centroid=[bytes(r[:W]).decode() for r in cen], centroid_dist=cd)
        return out

    def has_fold_long(self):
        return getattr(self.lib, "sf_fold_long", None) is not None

    def fold_long(self, seq, cons=None, structure=True):
        """fc = RNA.fold_compound(seq, md); fc.hc_add_from_db(cons); fc.mfe() for ONE sequence of 1..SF_MAX_LONG nt
        (ScanFold.py:1520-1539, --global_refold) -> (mfe_dcal, dot-bracket or None).  Raises ScanFoldHipError on a library
        without the entry point (there is no fallback)."""
        self._need(*_FOLD_LONG)
        return self._fold_record(self.lib.sf_fold_long, seq, cons, structure)

    def _fold_record(self, entry, seq, cons, structure):
        """entry = sf_fold_long or sf_fold_banded -> (mfe_dcal, dot-bracket or None)"""
        arr, L, c = _record(seq, cons)
        e = np.zeros(1, dtype=np.int32)
        db = np.zeros(L + 1, dtype=np.uint8) if structure else None
        self._check(entry(arr.ctypes.data, L, c, e.ctypes.data, None if db is None else db.ctypes.data))
        return int(e[0]), (bytes(db[:L]).decode() if structure else None)

    def fold_long_times(self):
        """-> (fill_ms, f5_ms, traceback_ms) of the last fold_long (device events)."""
        return tuple(self._times(_FOLD_LONG, fill_ms=_D, f5_ms=_D, trace_ms=_D).values())

    def has_fold_banded(self):
        return getattr(self.lib, "sf_fold_banded", None) is not None

    def fold_banded(self, seq, cons=None, structure=True):
        """fold_long under the resident base-pair span (set_max_bp_span(S), S >= 1) in banded tables (sf_fold_banded): ONE
        sequence of 1..SF_MAX_BANDED nt -> (mfe_dcal, dot-bracket or None), the bytes fold_long returns under the same span,
        from 12 L min(S, L) bytes of tables and min(S, L) fill launches.  Raises ScanFoldHipError where no span is set, and
        on a library without the entry point (there is no fallback)."""
        self._need(*_FOLD_BANDED)
        return self._fold_record(self.lib.sf_fold_banded, seq, cons, structure)

    def fold_banded_times(self):
        """-> dict(fill_ms, f5_ms, trace_ms, band, fill_launches) of the last fold_banded (device events; band = min(span, L))."""
        return self._times(_FOLD_BANDED, fill_ms=_D, f5_ms=_D, trace_ms=_D, band=_I, fill_launches=_I)

    def fold_banded_bytes(self, L, span):
        """the device memory fold_banded would allocate for L nucleotides under `span` (sf_fold_banded_bytes)"""
        self._need(*_FOLD_BANDED)
        n = ctypes.c_size_t()
        self._check(self.lib.sf_fold_banded_bytes(int(L), int(span), ctypes.byref(n)))
        return int(n.value)

    def has_fold_long_batch(self):
        return getattr(self.lib, "sf_fold_long_batch", None) is not None

    def fold_long_batch(self, seqs, cons=None, structure=False):
        """fold_long for many sequences of 1..SF_MAX_LONG nt, of any mix of lengths, side by side in the same launches
        (sf_fold_long_batch) -> int32 array of energies (dcal/mol), or (energies, [dot-bracket]) with structure=True.
        cons: None, or one item per sequence, each a constraint string of the sequence's length or None.  Raises
        ScanFoldHipError on a library without the entry point (there is no fallback)."""
        self._need(*_FOLD_LONG_BATCH)
        return self._fold_rows(self.lib.sf_fold_long_batch, seqs, cons, structure)

    def _fold_rows(self, entry, seqs, cons, structure):
        """entry = sf_fold_long_batch or sf_fold_banded_batch -> energies, or (energies, [dot-bracket])"""
        arr, lens, ld, c = _ragged_rows(seqs, cons)
        n = len(lens)
        e = np.zeros(n, dtype=np.int32)
        db = np.zeros((n, ld + 1), dtype=np.uint8) if structure else None
        self._check(entry(arr.ctypes.data, n, ld, lens.ctypes.data, None if c is None else c.ctypes.data,
                          e.ctypes.data, None if db is None else db.ctypes.data))
        if not structure:
            return e
        return e, [bytes(db[k, :lens[k]]).decode() for k in range(n)]

    def fold_long_batch_times(self):
        """-> dict(fill_ms, f5_ms, trace_ms, chunks) of the last fold_long_batch (device events, summed over its chunks)."""
        return self._times(_FOLD_LONG_BATCH, fill_ms=_D, f5_ms=_D, trace_ms=_D, chunks=_I)

    def set_long_batch_bytes(self, nbytes):
        """the device memory one chunk of fold_long_batch (and of fold_banded_batch and pf_long_batch) may take for its
        tables; 0 restores the default (8 GiB)"""
        self._need(*_FOLD_LONG_BATCH)
        self._check(self.lib.sf_set_long_batch_bytes(int(nbytes)))

    def has_fold_banded_batch(self):
        return getattr(self.lib, "sf_fold_banded_batch", None) is not None

    def fold_banded_batch(self, seqs, cons=None, structure=False):
        """fold_banded for many sequences of 1..SF_MAX_BANDED nt, of any mix of lengths, side by side in the same launches
        under the resident base-pair span (sf_fold_banded_batch) -> int32 array of energies (dcal/mol), or
        (energies, [dot-bracket]) with structure=True: every row the bytes fold_banded returns for it.  cons as for
        fold_long_batch.  Raises ScanFoldHipError where no span is set, and on a library without the entry point (there is no
        fallback)."""
        self._need(*_FOLD_BANDED_BATCH)
        return self._fold_rows(self.lib.sf_fold_banded_batch, seqs, cons, structure)

    def fold_banded_batch_times(self):
        """-> dict(fill_ms, f5_ms, trace_ms, chunks, fill_launches) of the last fold_banded_batch (device events, summed over
        its chunks; a chunk's fill launches are the widest band of its rows)."""
        return self._times(_FOLD_BANDED_BATCH, fill_ms=_D, f5_ms=_D, trace_ms=_D, chunks=_I, fill_launches=_I)

    def has_pf_long(self):
        return getattr(self.lib, "sf_pf_long", None) is not None

    def pf_long(self, seq, cons=None, mfe_hint=None):
        """fc.hc_add_from_db(cons); fc.pf(); fc.centroid(); fc.mean_bp_distance() (RNAfold -p -C, ScanFoldFunctions.py:758-772)
        for ONE sequence of 1..SF_MAX_LONG nt -> dict(dG, mean_bp_dist, centroid, centroid_dist), the keys of one pf_batch
        item.  mfe_hint: the sequence's MFE in dcal/mol (fold_long's), which sets the scale of the first attempt.  Raises
        ScanFoldHipError on a library without the entry point (there is no fallback)."""
        self._need(*_PF_LONG)
        return self._pf_record(self.lib.sf_pf_long, seq, cons, mfe_hint)

    def _pf_record(self, entry, seq, cons, mfe_hint):
        """entry = sf_pf_long or sf_pf_banded -> dict(dG, mean_bp_dist, centroid, centroid_dist)"""
        arr, L, c = _record(seq, cons)
        hint = None if mfe_hint is None else np.array([int(mfe_hint)], dtype=np.int32)
        out = np.zeros(3)
        cen = np.zeros(L + 1, dtype=np.uint8)
        self._check(entry(arr.ctypes.data, L, c, None if hint is None else hint.ctypes.data,
                          out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data, out[2:].ctypes.data))
        return dict(dG=float(out[0]), mean_bp_dist=float(out[1]), centroid=bytes(cen[:L]).decode(),
                    centroid_dist=float(out[2]))

    def pf_long_times(self):
        """-> dict(inside_ms, outside_ms, attempts, lns) of the last pf_long (device events; lns = the per-nucleotide scale)."""
        return self._times(_PF_LONG, inside_ms=_D, outside_ms=_D, attempts=_I, lns=_D)

    def has_pf_banded(self):
        return getattr(self.lib, "sf_pf_banded", None) is not None

    def pf_banded(self, seq, cons=None, mfe_hint=None):
        """pf_long under the resident base-pair span (set_max_bp_span(S), S >= 1) in banded tables (sf_pf_banded): ONE
        sequence of 1..SF_MAX_BANDED nt -> pf_long's dict, equal to pf_long's under the same span to rounding, from
        56 L min(S, L) bytes of tables.  The exterior loop carries its own exponents, so records past SF_MAX_LONG and
        records whose composition changes along their length work.  Raises ScanFoldHipError where no span is set, and on a
        library without the entry point (there is no fallback)."""
        self._need(*_PF_BANDED)
        return self._pf_record(self.lib.sf_pf_banded, seq, cons, mfe_hint)

    def pf_banded_times(self):
        """-> dict(inside_ms, outside_ms, attempts, lns, band, launches) of the last pf_banded (device events; lns = the band
        tables' per-nucleotide scale, band = min(span, L), launches = diagonal launches over all attempts)."""
        return self._times(_PF_BANDED, inside_ms=_D, outside_ms=_D, attempts=_I, lns=_D, band=_I, launches=_I)

    def pf_banded_bytes(self, L, span):
        """the device memory pf_banded would allocate for L nucleotides under `span` (sf_pf_banded_bytes)"""
        self._need(*_PF_BANDED)
        n = ctypes.c_size_t()
        self._check(self.lib.sf_pf_banded_bytes(int(L), int(span), ctypes.byref(n)))
        return int(n.value)

    def has_pf_banded_probs(self):
        return getattr(self.lib, "sf_pf_banded_probs", None) is not None

    def pf_banded_probs(self, seq, cons=None, mfe_hint=None, cutoff=0.01):
        """pf_banded with the base-pair probabilities brought out (sf_pf_banded_probs) -> pf_banded's dict, its four values
        bit for bit pf_banded's, plus
          unpaired  float64 (L,): the probability that nucleotide k + 1 is unpaired
          entropy   float64 (L,): its positional entropy in bits, -sum p log2 p over its pairs - unpaired log2 unpaired
          pairs     PAIR_PROB_DTYPE (n,): every pair with p >= cutoff (0 < cutoff <= 1), 1-based i < j, ascending in (i, j);
                    at most L * floor(1 / cutoff) / 2 of them.
        A span of at least the record's length gives the unrestricted probabilities.  Raises ScanFoldHipError where no span
        is set or the cutoff is out of range, and on a library without the entry point (there is no fallback)."""
        self._need(*_PF_BANDED_PROBS)
        arr, L, c = _record(seq, cons)
        hint = None if mfe_hint is None else np.array([int(mfe_hint)], dtype=np.int32)
        out = np.zeros(3)
        cen = np.zeros(L + 1, dtype=np.uint8)
        unp, ent = np.zeros(L), np.zeros(L)
        n = ctypes.c_size_t(0)
        self._check(self.lib.sf_pf_banded_probs(arr.ctypes.data, L, c, None if hint is None else hint.ctypes.data,
                                                float(cutoff), out[0:].ctypes.data, out[1:].ctypes.data, cen.ctypes.data,
                                                out[2:].ctypes.data, unp.ctypes.data, ent.ctypes.data, ctypes.byref(n)))
        pairs = np.zeros(n.value, dtype=PAIR_PROB_DTYPE)
        self._check(self.lib.sf_pf_probs_pairs(pairs.ctypes.data, n.value, ctypes.byref(n)))
        return dict(dG=float(out[0]), mean_bp_dist=float(out[1]), centroid=bytes(cen[:L]).decode(),
                    centroid_dist=float(out[2]), unpaired=unp, entropy=ent, pairs=pairs)

    def pf_banded_probs_times(self):
        """-> dict(extract_ms, n_pairs, extra_bytes) of the last pf_banded_probs: the device-event time of the extraction's
        launches (pf_banded_times has the passes before it), the length of the list, and the device bytes allocated on top
        of pf_banded_bytes."""
        return self._times(_PF_BANDED_PROBS, extract_ms=_D, n_pairs=_Z, extra_bytes=_Z)

    def has_mea_pairs(self):
        return getattr(self.lib, "sf_mea_pairs", None) is not None

    def mea_pairs(self, L, pairs, unpaired, gamma=1.0):
        """The maximum-expected-accuracy structure of a pair list (sf_mea_pairs; RNAfold -p --MEA gamma) -> (dot-bracket,
        score).  pairs: PAIR_PROB_DTYPE records (or anything np.asarray turns into them), 1-based i < j <= L, strictly
        ascending in (i, j), p in [0, 1]; unpaired: L values in [0, 1]; gamma > 0.  The structure maximises the sum of u over
        its unpaired positions plus 2 gamma p over its pairs, ties broken as include/scanfold_hip_long.h states, so structure
        and score are a function of the arguments alone.  Needs neither parameters nor a span.  Raises ScanFoldHipError on
        a bad argument and on a library without the entry point (there is no fallback)."""
        self._need(*_MEA_PAIRS)
        L = int(L)
        pr = np.ascontiguousarray(pairs, dtype=PAIR_PROB_DTYPE)
        unp = np.ascontiguousarray(unpaired, dtype=np.float64)
        if unp.shape != (max(L, 0),):
            raise ValueError("one unpaired probability per nucleotide")
        db = np.zeros(max(L, 0) + 1, dtype=np.uint8)
        score = ctypes.c_double(0.0)
        self._check(self.lib.sf_mea_pairs(L, pr.ctypes.data if len(pr) else None, len(pr), unp.ctypes.data, float(gamma),
                                          db.ctypes.data, ctypes.addressof(score)))
        return bytes(db[:L]).decode(), score.value

    def has_pf_banded_mea(self):
        return getattr(self.lib, "sf_pf_banded_mea", None) is not None

    def pf_banded_mea(self, seq, cons=None, mfe_hint=None, cutoff=0.01, gamma=1.0):
        """pf_banded_probs, then the maximum-expected-accuracy structure of its list and unpaired vector, formed on the device
        while they are there (sf_pf_banded_mea) -> pf_banded_probs's dict, every value bit for bit pf_banded_probs's, plus
          mea        the dot-bracket structure
          mea_score  its score: the sum of unpaired over its unpaired positions plus 2 gamma p over its pairs.
        gamma > 0 weighs pairs against unpaired positions: larger values give more pairs (RNAfold --MEA's gamma).
        mea_pairs on the returned pairs and unpaired gives the same structure and score.  Raises ScanFoldHipError where no
        span is set or cutoff or gamma is out of range, and on a library without the entry point (there is no fallback)."""
        self._need(*_PF_BANDED_MEA)
        arr, L, c = _record(seq, cons)
        hint = None if mfe_hint is None else np.array([int(mfe_hint)], dtype=np.int32)
        out = np.zeros(4)
        cen = np.zeros(L + 1, dtype=np.uint8)
        mea = np.zeros(L + 1, dtype=np.uint8)
        unp, ent = np.zeros(L), np.zeros(L)
        n = ctypes.c_size_t(0)
        self._check(self.lib.sf_pf_banded_mea(arr.ctypes.data, L, c, None if hint is None else hint.ctypes.data,
                                              float(cutoff), float(gamma), out[0:].ctypes.data, out[1:].ctypes.data,
                                              cen.ctypes.data, out[2:].ctypes.data, unp.ctypes.data, ent.ctypes.data,
                                              ctypes.byref(n), mea.ctypes.data, out[3:].ctypes.data))
        pairs = np.zeros(n.value, dtype=PAIR_PROB_DTYPE)
        self._check(self.lib.sf_pf_probs_pairs(pairs.ctypes.data, n.value, ctypes.byref(n)))
        return dict(dG=float(out[0]), mean_bp_dist=float(out[1]), centroid=bytes(cen[:L]).decode(),
                    centroid_dist=float(out[2]), unpaired=unp, entropy=ent, pairs=pairs, mea=bytes(mea[:L]).decode(),
                    mea_score=float(out[3]))

    def mea_times(self):
        """-> dict(fill_ms, ext_ms, trace_ms, band, fill_launches, extra_bytes) of the last mea_pairs or pf_banded_mea: device
        events of the three phases, the band of the list, and the device bytes the MEA allocated on top of what the call had
        anyway."""
        self._need("sf_mea_times", _MEA_PAIRS[1])
        vals = [_D(), _D(), _D(), _I(), _I(), _Z()]
        self._check(self.lib.sf_mea_times(*(ctypes.byref(v) for v in vals)))
        return {k: v.value for k, v in zip(("fill_ms", "ext_ms", "trace_ms", "band", "fill_launches", "extra_bytes"), vals)}

    def has_pf_long_batch(self):
        return getattr(self.lib, "sf_pf_long_batch", None) is not None

    def pf_long_batch(self, seqs, cons=None, mfe_hints=None):
        """pf_long for many sequences of 1..SF_MAX_LONG nt, of any mix of lengths, side by side in the same launches
        (sf_pf_long_batch) -> a list of pf_long's dicts with two more keys, lns (the row's final per-nucleotide scale) and
        attempts (its inside passes).  cons / mfe_hints: None, or one item per sequence, each a constraint string of the
        sequence's length / the sequence's MFE in dcal/mol, or None.  Every row equals pf_long of that row bit for bit.
        Raises ScanFoldHipError on a library without the entry point (there is no fallback)."""
        self._need(*_PF_LONG_BATCH)
        arr, lens, ld, c = _ragged_rows(seqs, cons)
        n = len(lens)
        h = None
        if mfe_hints is not None:
            mfe_hints = list(mfe_hints)
            if len(mfe_hints) != n:
                raise ValueError("one MFE hint (an energy in dcal/mol or None) per sequence")
            if any(x is not None for x in mfe_hints):
                h = np.array([SF_PF_LONG_NO_HINT if x is None else int(x) for x in mfe_hints], dtype=np.int32)
        out = np.zeros(n, dtype=PF_LONG_ROW_DTYPE)
        cen = np.zeros((n, ld + 1), dtype=np.uint8)
        self._check(self.lib.sf_pf_long_batch(arr.ctypes.data, n, ld, lens.ctypes.data, None if c is None else c.ctypes.data,
                                              None if h is None else h.ctypes.data, out.ctypes.data, cen.ctypes.data))
        return [dict(dG=float(out["ens_dG"][k]), mean_bp_dist=float(out["mean_bp_dist"][k]),
                     centroid=bytes(cen[k, :lens[k]]).decode(), centroid_dist=float(out["centroid_dist"][k]),
                     lns=float(out["lns"][k]), attempts=int(out["attempts"][k])) for k in range(n)]

    def pf_long_batch_times(self):
        """-> dict(inside_ms, outside_ms, chunks, inside_passes) of the last pf_long_batch (device events, summed over its
        chunks; inside_passes = chunks when no row needed another scale)."""
        return self._times(_PF_LONG_BATCH, inside_ms=_D, outside_ms=_D, chunks=_I, inside_passes=_I)

    # -- duplex folds and the LRI scan (include/scanfold_hip_duplex.h) --
    def has_duplex(self):
        return all(getattr(self.lib, name, None) is not None for name in _DUPLEX_EXPORTS)

    def duplex_batch(self, s1, s2, structure=True):
        """RNA.duplexfold(s1[p], s2[p]) for every p (ScanFold.py:785) -> dict(energy int32 dcal/mol or SF_DUPLEX_NONE,
        i, j int32 (duplexT's .i / .j), structure [str] or None).  Strands of 0..SF_DUPLEX_MAX_LEN nucleotides, mixed freely."""
        self._need(*_DUPLEX)
        a = [_ascii(s) for s in s1]
        b = [_ascii(s) for s in s2]
        if len(a) != len(b):
            raise ValueError("one strand 2 per strand 1")
        n = len(a)
        ld = max([1] + [len(s) for s in a] + [len(s) for s in b])
        if ld > SF_DUPLEX_MAX_LEN:
            raise ValueError("a duplex strand is at most %d nucleotides" % SF_DUPLEX_MAX_LEN)
        m1, m2 = _pad(a, ld), _pad(b, ld)
        l1 = np.array([len(s) for s in a], dtype=np.int32)
        l2 = np.array([len(s) for s in b], dtype=np.int32)
        e, ri, rj = (np.zeros(n, dtype=np.int32) for _ in range(3))
        st = np.zeros((n, SF_DUPLEX_STRUCT_LEN), dtype=np.uint8) if structure else None
        self._check(self.lib.sf_duplex_batch(m1.ctypes.data, m2.ctypes.data, n, ld, l1.ctypes.data, l2.ctypes.data,
                                             e.ctypes.data, ri.ctypes.data, rj.ctypes.data,
                                             None if st is None else st.ctypes.data))
        return dict(energy=e, i=ri, j=rj,
                    structure=None if st is None else [bytes(r).split(b"\0")[0].decode() for r in st])

    def lri_grid(self, L, kmer, step):
        """-> (n_j, n_k): j_win = jx * step, k_win = kx * step of the reference's two loops (ScanFold.py:774,780)"""
        self._need(*_DUPLEX)
        nj, nk = ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.sf_lri_grid(int(L), int(kmer), int(step), ctypes.byref(nj), ctypes.byref(nk)))
        return nj.value, nk.value

    def lri_scan(self, seq, kmer, step, cutoff_dcal, max_hits=1 << 20, dense=False):
        """The all-pairs k-mer duplex scan (ScanFold.py:773-812).  Compacted (default): the pairs with Emin < cutoff_dcal as
        a LRI_HIT_DTYPE array sorted by (j_win, k_win); more than max_hits raises ScanFoldHipError.  dense=True: dict(energy,
        i, j) of int32 (n_j, n_k) arrays, SF_DUPLEX_SKIPPED where the distance test fails (small records: tests)."""
        self._need(*_DUPLEX)
        s = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
        if dense:
            nj, nk = self.lri_grid(len(s), kmer, step)
            e, ri, rj = (np.zeros((nj, nk), dtype=np.int32) for _ in range(3))
            if nj and nk:
                self._check(self.lib.sf_lri_scan(s.ctypes.data, len(s), kmer, step, int(cutoff_dcal), 0, None, None,
                                                 e.ctypes.data, ri.ctypes.data, rj.ctypes.data))
            return dict(energy=e, i=ri, j=rj)
        hits = np.zeros(max(int(max_hits), 1), dtype=LRI_HIT_DTYPE)
        n = ctypes.c_int64(0)
        rc = self.lib.sf_lri_scan(s.ctypes.data, len(s), kmer, step, int(cutoff_dcal), int(max_hits), hits.ctypes.data,
                                  ctypes.byref(n), None, None, None)
        if rc == SF_ERR_DUPLEX_HITS:
            raise ScanFoldHipError("%s: %d pairs are below the cutoff, max_hits is %d"
                                   % (self.lib.sf_strerror(rc).decode(), n.value, max_hits))
        self._check(rc)
        return hits[:n.value].copy()

    def lri_scan_time(self):
        """-> (ms of the scan kernels of the last lri_scan by device events, duplexes they folded)"""
        self._need(*_DUPLEX)
        ms, nd = ctypes.c_double(), ctypes.c_int64()
        self._check(self.lib.sf_lri_scan_time(ctypes.byref(ms), ctypes.byref(nd)))
        return ms.value, nd.value

    def lri_background(self, seq, kmer, j_win, k_win, r, kind, seed, rows=False):
        """cofold_energies(frag, [dup_frag] + scramble(dup_frag, r, type)) for every hit (ScanFold.py:813-817) -> int32
        (n_hits, r+1) energies; rows=True: (energies, rows1, rows2), the folded strands as uint8 codes (n_hits, r+1, kmer)."""
        self._need(*_DUPLEX)
        s = np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
        jw = np.ascontiguousarray(j_win, dtype=np.int32)
        kw = np.ascontiguousarray(k_win, dtype=np.int32)
        if jw.shape != kw.shape or jw.ndim != 1:
            raise ValueError("one k_win per j_win")
        n = len(jw)
        en = np.zeros((n, r + 1), dtype=np.int32)
        r1 = np.zeros((n, r + 1, kmer), dtype=np.uint8) if rows else None
        r2 = np.zeros((n, r + 1, kmer), dtype=np.uint8) if rows else None
        self._check(self.lib.sf_lri_background(s.ctypes.data, len(s), int(kmer), jw.ctypes.data, kw.ctypes.data, n, int(r),
                                               int(kind), ctypes.c_uint64(seed), en.ctypes.data,
                                               None if r1 is None else r1.ctypes.data,
                                               None if r2 is None else r2.ctypes.data))
        return (en, r1, r2) if rows else en

    def shuffle_windows(self, transcript, W, step, win_begin, n_win, r, kind, seed):
        tr = np.frombuffer(transcript.encode("ascii") if isinstance(transcript, str) else bytes(transcript),
                           dtype=np.uint8)
        out = np.empty((n_win * (r + 1), W), dtype=np.uint8)
        self._check(self.lib.sf_shuffle_windows(tr.ctypes.data, len(tr), W, step, win_begin, n_win, r, kind,
                                                ctypes.c_uint64(seed), out.ctypes.data))
        return out

    def scan(self, transcript, W, step, win_begin, n_win, r, kind, seed, flags=0, raw=False):
        """-> dict(energies int32 (n_win, r+1), structure [str], centroid [str], ens_div, ens_dG);
        raw=True leaves structure / centroid as the uint8 arrays (n_win, W+1) the library filled."""
        tr = np.frombuffer(transcript.encode("ascii") if isinstance(transcript, str) else bytes(transcript),
                           dtype=np.uint8)
        en = np.empty((n_win, r + 1), dtype=np.int32)
        db = np.zeros((n_win, W + 1), dtype=np.uint8)
        cen = np.zeros((n_win, W + 1), dtype=np.uint8)
        div = np.zeros(n_win)
        dG = np.zeros(n_win)
        self._check(self.lib.sf_scan(tr.ctypes.data, len(tr), W, step, win_begin, n_win, r, kind,
                                     ctypes.c_uint64(seed), flags, en.ctypes.data, db.ctypes.data, cen.ctypes.data,
                                     div.ctypes.data, dG.ctypes.data))
        if raw:
            return dict(energies=en, structure=db, centroid=cen, ens_div=div, ens_dG=dG)
        return dict(energies=en, structure=[bytes(x[:W]).decode() for x in db],
                    centroid=[bytes(x[:W]).decode() for x in cen], ens_div=div, ens_dG=dG)

    def tabulate_pairs(self, structures, starts, z, mfe, ed, W=None, row_stride=None, on_device=False):
        """Base-pair tabulation of a scan table (ScanFold-Fold.py:583-682,704-760) -> dict of per-group arrays
        k, j (j == k: unpaired), windows, first_window, sum_z, sum_mfe, sum_ed, ordered by k then first window.
        structures: list of W-char str, a uint8 array (n, >= W) (e.g. the raw (n, W+1) table of scan(raw=True)), or —
        with on_device=True, W and row_stride given — the device pointer of the table sf_scan_dev wrote."""
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        n = len(starts)
        z, mfe, ed = (np.ascontiguousarray(v, dtype=np.float64) for v in (z, mfe, ed))
        if not (len(z) == len(mfe) == len(ed) == n):
            raise ValueError("one z-score, MFE and ED per window")
        if on_device:
            ptr, keep = int(structures), None
        else:
            keep = seqs_to_array(structures) if not isinstance(structures, np.ndarray) else np.ascontiguousarray(structures, dtype=np.uint8)
            if keep.ndim != 2 or keep.shape[0] != n:
                raise ValueError("one structure row per window")
            row_stride = keep.shape[1]
            W = row_stride if W is None else W
            ptr = keep.ctypes.data
        ng = ctypes.c_int64(0)
        self._check(self.lib.sf_tabulate_pairs(ptr, int(row_stride), 1 if on_device else 0, n, int(W), starts.ctypes.data,
                                               z.ctypes.data, mfe.ctypes.data, ed.ctypes.data, ctypes.byref(ng)))
        g = int(ng.value)
        out = dict(k=np.empty(g, np.int32), j=np.empty(g, np.int32), windows=np.empty(g, np.int32),
                   first_window=np.empty(g, np.int32), sum_z=np.empty(g), sum_mfe=np.empty(g), sum_ed=np.empty(g))
        self._check(self.lib.sf_tabulate_fetch(*(out[key].ctypes.data for key in
                                                 ("k", "j", "windows", "first_window", "sum_z", "sum_mfe", "sum_ed"))))
        return out

    # -- device-buffer entry points (pointers are ints, e.g. torch.Tensor.data_ptr(); stream 0 = library stream) --
    def mfe_batch_dev(self, d_seqs, n, W, d_out, stream=0):
        self._check(self.lib.sf_mfe_batch_dev(d_seqs, n, W, d_out, stream))

    def scan_dev(self, d_transcript, L, W, step, win_begin, n_win, r, kind, seed, flags, d_energies, d_structure,
                 d_centroid, d_ens_div, d_ens_dG, stream=0):
        self._check(self.lib.sf_scan_dev(d_transcript, L, W, step, win_begin, n_win, r, kind, ctypes.c_uint64(seed),
                                         flags, d_energies, d_structure, d_centroid, d_ens_div, d_ens_dG, stream))

    def last_status(self):
        """0, or SF_ERR_INTERNAL (-8) if a traceback of an asynchronous call failed; waits for the device."""
        rc = self.lib.sf_last_status()
        if rc not in (0, -8):
            self._check(rc)
        return rc

    def prof_stop(self):
        self._check(self.lib.sf_prof_stop())

    def set_kernel_mode(self, mode):
        self._check(self.lib.sf_set_kernel_mode(int(mode)))

    def set_max_bp_span(self, span):
        """RNA.md().max_bp_span (ScanFold.py:214-215): pairs (i, j) with j - i + 1 > span do not exist; <= 0 = no limit."""
        self._check(self.lib.sf_set_max_bp_span(int(span or 0)))
        self.max_bp_span = int(span or 0) if int(span or 0) > 0 else 0

    def prof_reset(self):
        self._check(self.lib.sf_prof_reset())

    def prof_get(self):
        ms = ctypes.c_double()
        nl = ctypes.c_int64()
        nf = ctypes.c_int64()
        self._check(self.lib.sf_prof_get(ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(nf)))
        return ms.value, nl.value, nf.value


_engine = None


def get_engine(device=None):
    """Process-wide engine on LOCAL_RANK's GPU (or `device`)."""
    global _engine
    if _engine is None:
        if device is None:
            # SCANFOLD_DEVICE: several ranks on one GPU (the 2-rank test on a 1-GPU box); default: the rank's own GPU
            device = int(os.environ.get("SCANFOLD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        # SCANFOLD_LIB_PATH: another build of the same C ABI (build variants; tests/emul's CPU build in the no-GPU suite)
        _engine = Engine(device=device, lib_path=os.environ.get("SCANFOLD_LIB_PATH", LIB_PATH))
        _params.warn_if_reconstructed(_engine.params)  # the shipped table is not ViennaRNA's: say so once
    return _engine

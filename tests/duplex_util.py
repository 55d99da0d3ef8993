"""TEST-ONLY ctypes wrapper of tests/duplex_ref (the plain-C restatement of the duplex model), built on demand, and the
literal transcription of the reference's k-mer loops (ScanFold.py:773-783,1019-1024)."""
import ctypes
import os
import subprocess

import numpy as np

from scanfold_amd import _lib as _sf

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "duplex_ref")
_LIB = os.path.join(_DIR, "libduplex_ref.so")
NONE = _sf.SF_DUPLEX_NONE  # (include/scanfold_hip_duplex.h, read by the package)
SKIPPED = _sf.SF_DUPLEX_SKIPPED
STRUCT_LEN = _sf.SF_DUPLEX_STRUCT_LEN
THREADS = min(16, os.cpu_count() or 1)
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", _DIR, "-s"])
        _lib = ctypes.CDLL(_LIB)
        _lib.dr_fold.restype = ctypes.c_int
    return _lib


def set_params(paramset):
    blob = paramset.blob()
    lib().dr_set_params(blob)


def _bytes(s):
    return s if isinstance(s, (bytes, bytearray)) else str(s).encode("ascii")


def fold(s1, s2):
    """-> (Emin dcal or NONE, i, j, structure)"""
    a, b = _bytes(s1), _bytes(s2)
    ri, rj = ctypes.c_int(), ctypes.c_int()
    st = ctypes.create_string_buffer(STRUCT_LEN)
    e = lib().dr_fold(a, len(a), b, len(b), ctypes.byref(ri), ctypes.byref(rj), st)
    return e, ri.value, rj.value, st.value.decode()


def pack(seqs, ld):
    arr = np.zeros((len(seqs), ld), dtype=np.uint8)
    for p, s in enumerate(seqs):
        b = _bytes(s)
        arr[p, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return arr, np.array([len(s) for s in seqs], dtype=np.int32)


def batch(s1, s2, structures=True, threads=THREADS):
    """lists of str -> (e, i, j int32 arrays, [structure] or None)"""
    n = len(s1)
    ld = max([1] + [len(s) for s in s1] + [len(s) for s in s2])
    a, l1 = pack(s1, ld)
    b, l2 = pack(s2, ld)
    e, ri, rj = (np.zeros(n, dtype=np.int32) for _ in range(3))
    st = np.zeros((n, STRUCT_LEN), dtype=np.uint8) if structures else None
    lib().dr_batch(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), n, ld,
                   l1.ctypes.data_as(ctypes.c_void_p), l2.ctypes.data_as(ctypes.c_void_p),
                   e.ctypes.data_as(ctypes.c_void_p), ri.ctypes.data_as(ctypes.c_void_p),
                   rj.ctypes.data_as(ctypes.c_void_p), None if st is None else st.ctypes.data_as(ctypes.c_void_p),
                   STRUCT_LEN, threads)
    return e, ri, rj, (None if st is None else [bytes(r).split(b"\0")[0].decode() for r in st])


def pairs(seq, kmer, jw, kw, threads=THREADS):
    """k-mer pairs of one record -> (e, i, j)"""
    s = np.frombuffer(_bytes(seq), dtype=np.uint8)
    jw = np.ascontiguousarray(jw, dtype=np.int32)
    kw = np.ascontiguousarray(kw, dtype=np.int32)
    n = len(jw)
    e, ri, rj = (np.zeros(n, dtype=np.int32) for _ in range(3))
    lib().dr_pairs(s.ctypes.data_as(ctypes.c_void_p), len(s), kmer, jw.ctypes.data_as(ctypes.c_void_p),
                   kw.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(n), e.ctypes.data_as(ctypes.c_void_p),
                   ri.ctypes.data_as(ctypes.c_void_p), rj.ctypes.data_as(ctypes.c_void_p), threads)
    return e, ri, rj


def reference_loops(L, kmer, step):
    """The (j_win, k_win) the reference folds, in its order: its two `while` loops and its distance test, transcribed."""
    out = []
    j_win = 0
    while j_win == 0 or j_win <= (L - kmer + 1):
        start_nucleotide = j_win
        k_win = 0
        while k_win == 0 or k_win <= (L - kmer):
            if ((k_win + 3) < (start_nucleotide - kmer)) or (k_win > (start_nucleotide + kmer + 3)):
                out.append((j_win, k_win))
            k_win += step
        j_win += step
    return out


def dense_reference(seq, kmer, step):
    """-> dict (j_win, k_win) -> (e, i, j) over reference_loops"""
    pl = reference_loops(len(seq), kmer, step)
    if not pl:
        return {}
    e, ri, rj = pairs(seq, kmer, [p[0] for p in pl], [p[1] for p in pl])
    return {p: (int(e[x]), int(ri[x]), int(rj[x])) for x, p in enumerate(pl)}

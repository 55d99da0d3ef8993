"""The duplex reference of the test suite (tests/duplex_ref) pinned by exhaustive enumeration: for small strands every
duplex — every ordered chain of inter-strand pairs with interior loops of at most 30 unpaired nucleotides — is scored
with tests/py_model.Model, which shares no code with the library or the reference, and the minimum must be the reference's
energy; the reference's structure must evaluate to it.  Default and randomised tables."""
import itertools
from unittest import mock

import numpy as np
import pytest

import duplex_util as du
import py_model
from scanfold_amd import params


def chains(s1, s2):
    """every duplex as a list of (i, j) pairs, 1-based, i ascending and j descending, loops <= 30"""
    n1, n2 = len(s1), len(s2)
    can = {(i, j) for i in range(1, n1 + 1) for j in range(1, n2 + 1) if (s1[i - 1], s2[j - 1]) in py_model.PAIR}

    def grow(chain):
        yield chain
        k, l = chain[-1]
        for i in range(k + 1, n1 + 1):
            for j in range(l - 1, 0, -1):
                if (i, j) in can and (i - k - 1) + (l - j - 1) <= 30:
                    yield from grow(chain + [(i, j)])
    for first in sorted(can):
        yield from grow([first])


def score(model, dinit, s1, s2, chain):
    """dcal/mol of one duplex: DuplexInit, the two exterior stem terms (dangles = 2) and the loops between the pairs"""
    n1, n2 = len(s1), len(s2)
    cat = s1 + s2
    code = lambda ch: py_model.CODE[ch]
    k, l = chain[0]  # outermost: 5' neighbour on strand 1, 3' neighbour on strand 2
    e = dinit + model._stem("mismatchExt", py_model.PAIR[(s1[k - 1], s2[l - 1])],
                            code(s1[k - 2]) if k > 1 else None, code(s2[l]) if l < n2 else None)
    for (k, l), (i, j) in zip(chain, chain[1:]):
        e += model.interior(cat, k, n1 + l, i, n1 + j)
    i, j = chain[-1]  # innermost: read from strand 2's side
    e += model._stem("mismatchExt", py_model.RTYPE[py_model.PAIR[(s1[i - 1], s2[j - 1])]],
                     code(s2[j - 2]) if j > 1 else None, code(s1[i]) if i < n1 else None)
    return int(round(e))


def chain_of(structure, ri, rj):
    left, right = structure.split("&")
    op = [ri - len(left) + 1 + x for x, ch in enumerate(left) if ch == "("]
    cl = [rj + x for x, ch in enumerate(right) if ch == ")"]
    assert len(op) == len(cl)
    return list(zip(op, cl[::-1]))


def cases():
    rng = np.random.default_rng(5)
    out = [("A", "U"), ("G", "A"), ("AAAA", "CCCC"), ("G", "CCUC"), ("GGGGGG", "CCCCCC"), ("GCGCGCG", "GCGCGCG"),
           ("GGNGG", "CCNCC"), ("NNN", "NNN"), ("ACGUACG", "U"), ("GGGUGG", "CCGCC")]
    for n in range(40):
        al = ("GC", "ACGU", "ACGUN", "GU")[n % 4]
        a, b = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        out.append(("".join(al[k] for k in rng.integers(0, len(al), a)), "".join(al[k] for k in rng.integers(0, len(al), b))))
    return out


@pytest.mark.parametrize("seed", [None, 1, 2])
def test_reference_is_the_exhaustive_minimum(seed):
    p = params.default_params() if seed is None else params.random_params(seed)
    du.set_params(p)
    model = py_model.Model(p, p.temperature, "mfe")
    dinit = int(p.rec["DuplexInit"])
    ties = 0
    with mock.patch.dict(py_model.CODE, {"N": 0}):
        for s1, s2 in cases():
            e, ri, rj, st = du.fold(s1, s2)
            scores = [score(model, dinit, s1, s2, c) for c in chains(s1, s2)]
            if not scores:
                assert (e, ri, rj, st) == (du.NONE, 0, 0, "&"), (s1, s2)
                continue
            assert e == min(scores), (s1, s2, e, min(scores))
            ties += scores.count(min(scores)) > 1
            ch = chain_of(st, ri, rj)
            assert score(model, dinit, s1, s2, ch) == e, (s1, s2, st)
            # the record: .i / .j are one past the innermost pair where the strand goes on
            i_in, j_in = ch[-1]
            assert ri == min(i_in + 1, len(s1)) and rj == max(j_in - 1, 1)
    assert ties > 0 or seed is not None  # with the default tables the GC-rich cases do tie

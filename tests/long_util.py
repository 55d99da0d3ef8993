"""Helpers shared by the whole-record fold tests (tests/test_long_fold.py on the CPU, tests/test_gpu_long_fold.py on the GPU).

The oracle's fill is O(L^3) and needs (L+2)^2 ints per table, so it cannot fold a genome-length record itself.
`separated_record` builds records it can still answer exactly: with max_bp_span = S, blocks joined by separators of at least S
bases that cannot pair (runs of N, or random bases marked 'x') fold independently.  No pair crosses a separator, unpaired
exterior bases cost nothing, and with dangles = 2 a stem's exterior term reads only its two neighbours.  So the record's MFE
is the sum of the blocks' MFEs, each block folded with one flanking separator base on each inner side (marked 'x'), and the
record's structure is the blocks' structures joined with '.' over the separators, byte for byte: f5 inside a block is the
block's own f5 plus a constant, so the traceback makes the same choices."""
import numpy as np

PAIRS = {("A", "U"), ("U", "A"), ("G", "C"), ("C", "G"), ("G", "U"), ("U", "G")}
COMP = str.maketrans("ACGU", "UGCA")


def rand_seq(rng, L, alphabet="ACGU"):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), L))


def with_oracle_constraint(oracle, cons, fn):
    oracle.set_constraint(cons)
    try:
        return fn()
    finally:
        oracle.set_constraint(None)


def pair_table(db):
    """{i: j, j: i} over the pairs of a dot-bracket string (0-based)"""
    pt, stack = {}, []
    for k, ch in enumerate(db):
        if ch == "(":
            stack.append(k)
        elif ch == ")":
            o = stack.pop()
            pt[o], pt[k] = k, o
    return pt


def formed_type7(seq, cons, db):
    """the bracket pairs of the constraint between non-complementary bases that db forms"""
    pt, cpt = pair_table(db), pair_table(cons.replace("x", ".").replace("<", ".").replace(">", "."))
    return [(i, j) for i, j in cpt.items() if i < j and pt.get(i) == j and (seq[i], seq[j]) not in PAIRS]


def hairpin_rich(rng, L):
    """random sequence of exactly L nt with a GAAA-capped hairpin of 6..11 stacked pairs every 150..400 nt"""
    out, n = [], 0
    while n < L:
        stem = rand_seq(rng, int(rng.integers(6, 12)))
        out.append(rand_seq(rng, int(rng.integers(150, 400))) + stem + "GAAA" + stem[::-1].translate(COMP))
        n += len(out[-1])
    return "".join(out)[:L]


def multiloop_rich(rng, L):
    """random sequence of exactly L nt with a planted multiloop every 5..30 nt: a G-C stem closing a GAA- or GAAA-capped hairpin
    and the single pair G(AAA)C side by side, in either order, with no unpaired base between them or next to the closing pair.
    Under short_hairpin_params the optimum keeps the single pair, which the split DML[i][j] = min_k fML[i][k] + fML[k+1][j]
    then finds only at its first or last k.  The two loop sizes give the split ranges both parities, so an unrolled split
    loop's odd tail step is needed too."""
    out, n = [], 0
    while n < L:
        a, b = rand_seq(rng, 5, "GC"), rand_seq(rng, int(rng.integers(3, 6)), "GC")
        br = b + ("GAAA" if rng.random() < 0.5 else "GAA") + b[::-1].translate(COMP)
        inner = br + "GAAAC" if rng.random() < 0.5 else "GAAAC" + br
        out.append(rand_seq(rng, int(rng.integers(5, 31))) + a + inner + a[::-1].translate(COMP))
        n += len(out[-1])
    return "".join(out)[:L]


def short_hairpin_params():
    """the default set with hairpins of 3 and 4 unpaired bases cheap (-3 / -2 kcal/mol), so that multiloops keep branches
    of a single pair; blocks from multiloop_rich fold with them"""
    from scanfold_amd import params
    p = params.default_params()
    p.rec["hairpin"][3] = -300
    p.rec["hairpin"][4] = -200
    return p


def block_constraint(s, rng, S, close_at_end=False):
    """-> (s', c): 'x < >' marks on a tenth of the block, and a bracket pair of non-complementary bases (type 7) no wider than
    S closing a helix of eight G-C pairs planted into s, whose outer pair is bracketed too (so the type-7 pair forms).
    close_at_end: the type-7 pair closes within the block's last 6 bases."""
    L = len(s)
    c = ["."] * L
    for k in rng.choice(L, max(4, L // 10), replace=False):
        c[k] = "x<>"[k % 3]
    w = min(S, L - 4) - 1  # j - i of the type-7 pair
    starts = range(L - 3 - w, L - 8 - w, -1) if close_at_end else range(2, L - 2 - w)
    a = next(i for i in starts if (s[i], s[i + w]) not in PAIRS)
    stem = rand_seq(rng, 8, "GC")
    s = s[:a + 1] + stem + s[a + 9:a + w - 8] + stem[::-1].translate(COMP) + s[a + w:]
    c[a + 1:a + 9] = c[a + w - 8:a + w] = ["."] * 8
    c[a], c[a + w], c[a + 1], c[a + w - 1] = "(", ")", "(", ")"
    return s, "".join(c)


def separated_record(oracle, block_lens, kind, S, seed, cons_blocks=(), outer_pair=False, fill=rand_seq):
    """-> (seq, cons, e, db): a record of blocks of the given lengths joined by separators of S bases, and its exact MFE and
    structure under max_bp_span = S from the oracle folds of the blocks.

    kind 'N': the separators are runs of N;  kind 'x': random bases marked 'x' in the constraint.
    cons_blocks: indices of the blocks that get block_constraint marks (the last block's type-7 pair closes at its end).
    outer_pair: a bracket pair (1, L) in the constraint; the span forbids it, so the blocks see positions 1 and L as 'x'.
    fill(rng, n): the sequence of a block (rand_seq, hairpin_rich, multiloop_rich).
    cons is None when the record needs no constraint (kind 'N', no marks)."""
    assert kind in ("N", "x")
    rng = np.random.default_rng(seed)
    nb = len(block_lens)
    blocks = [fill(rng, n) for n in block_lens]
    bcons = ["." * n for n in block_lens]
    for b in cons_blocks:
        blocks[b], bcons[b] = block_constraint(blocks[b], rng, S, close_at_end=(b == nb - 1))
    seps = [("N" * S) if kind == "N" else rand_seq(rng, S) for _ in range(nb - 1)]
    sep_cons = ("." if kind == "N" else "x") * S
    seq = blocks[0] + "".join(sep + blk for sep, blk in zip(seps, blocks[1:]))
    cons = bcons[0] + "".join(sep_cons + bc for bc in bcons[1:])
    if outer_pair:
        cons = "(" + cons[1:-1] + ")"
        bcons[0] = "x" + bcons[0][1:]
        bcons[-1] = bcons[-1][:-1] + "x"
    if kind == "N" and not cons_blocks and not outer_pair:
        cons = None
    e, dbs = 0, []
    oracle.set_max_bp_span(S)
    try:
        for b in range(nb):
            left = seps[b - 1][-1:] if b > 0 else ""
            right = seps[b][:1] if b < nb - 1 else ""
            bs = left + blocks[b] + right
            bc = "x" * len(left) + bcons[b] + "x" * len(right)
            db, eb = with_oracle_constraint(oracle, bc, lambda: oracle.mfe(bs))
            e += eb
            dbs.append(db[len(left):len(db) - len(right)])
    finally:
        oracle.set_max_bp_span(0)
    db = dbs[0] + "".join("." * S + d for d in dbs[1:])
    assert len(seq) == len(db) == sum(block_lens) + S * (nb - 1)
    return seq, cons, e, db


def lengths_summing_to(rng, total, S, lo, hi):
    """block lengths in lo..hi whose blocks and separators of S bases make a record of exactly `total` nt"""
    out, n = [], 0
    while True:
        k = int(rng.integers(lo, hi + 1))
        rest = total - n - k
        if rest < lo + S:  # the last block takes what is left (lo <= it <= hi + lo + S)
            out.append(total - n)
            return out
        out.append(k)
        n += k + S


def hairpin_record(rng, s, flank=25):
    """(seq, cons, db): A/C flanks around ten G-C pairs bracketed '((((((((((' ... '))))))))))' that close a run of s bases
    marked 'x'.  The ten bracketed pairs are the only pairs the constraint allows: a bracketed base pairs with its partner
    or not at all, the run is 'x', and the flanks' A and C have no other partner.  db forms all ten, the stem with a hairpin
    of size s.  That this is the MFE rests on the stem's stacking outweighing the larger hairpin left by dropping inner
    pairs; the oracle's fold confirms it up to s = 1 000, and past that a GPU result other than db fails the test."""
    stem = rand_seq(rng, 10, "GC")
    seq = rand_seq(rng, flank, "AC") + stem + rand_seq(rng, s) + stem[::-1].translate(COMP) + rand_seq(rng, flank, "AC")
    cons = "." * flank + "(" * 10 + "x" * s + ")" * 10 + "." * flank
    return seq, cons, cons.replace("x", ".")

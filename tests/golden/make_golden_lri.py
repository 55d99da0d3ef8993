"""Generator of tests/golden/lri_cases.json: runs the reference's own per-pair lines of its LRI loop (ScanFold.py:785-1015)
at generation time, with RNA.duplexfold / scramble / cofold_energies stubbed to return canned records, and stores only the
inputs and what those lines produced (the `.LRI.out` row and the base pairs they put into bp_dict).  Nothing of the
reference's text goes into the repository.

    python tests/golden/make_golden_lri.py /path/to/reference/ScanFold.py
"""
import io
import json
import os
import sys
import textwrap
import types

# name, frag, dup_frag, j_win, k_win, canned duplex (energy_dcal, i, j, structure), canned z-score
CASES = [
    ("downstream: plain helix", "GGGGAAACCCGGAUUACGCA", "UGCGUAAUCCGGGUUUCCCC", 10, 200, (-3010, 20, 1, "((((((((((((((((((((&))))))))))))))))))))"), -3.21),
    ("upstream: plain helix", "GGGGAAACCCGGAUUACGCA", "UGCGUAAUCCGGGUUUCCCC", 300, 40, (-3010, 20, 1, "((((((((((((((((((((&))))))))))))))))))))"), -2.5),
    ("bulge: downstream", "ACGGGAUCCGAUCGAUCGAA", "UUCGAUCGAUCGGAACCCGA", 5, 90, (-2670, 19, 2, ".(((((((.(((((((((&))))))))))).)))))."), -4.0),
    ("bulge: interior loop, inside the strands", "AAGGCCAAGGCCUUAAGGAA", "AAUUCCAAGGCCAAGGCCAA", 0, 60, (-2590, 17, 4, ".((((((..((((((.&.))))))...)))))).",), 0.37),
    ("strand ends: both ends paired", "GCGCGCGCGCGCGCGCGCGC", "GCGCGCGCGCGCGCGCGCGC", 7, 100, (-4000, 20, 1, "((((((((((((((((((((&))))))))))))))))))))"), -1.0),
    ("strand ends: first pair at the 5' end of strand 1", "GGGGGAAAAAAAAAAAAAAA", "AAAAAAAAAAAAAAACCCCC", 50, 120, (-2600, 6, 15, "(((((.&.)))))"), 9.99),
    ("downstream: z-score filtered out", "GGGGGAAAAAAAAAAAAAAA", "AAAAAAAAAAAAAAACCCCC", 50, 120, (-2600, 6, 15, "(((((.&.)))))"), 10.0),
]


def main(ref_path):
    lines = open(ref_path).read().split("\n")[784:1015]  # :785-1015, the body of the distance test
    body = textwrap.dedent("\n".join(lines))
    code = compile("def per_pair(frag, dup_frag, j_win, k_win, start_nucleotide, lri_cutoff, randomizations, type, "
                   "zscore_total, bp_dict, lri_file, kmer_step_size):\n" + textwrap.indent(body, "    ") + "\n    return locals()\n",
                   "reference-lines", "exec")
    out = []
    for name, frag, dup, jw, kw, (e, i, j, st), z in CASES:
        class NucPair:
            def __init__(self, inuc, icoord, jnuc, jcoord, zscore, mfe, ed):
                self.v = (inuc, icoord, jnuc, jcoord)
        rna = types.SimpleNamespace(duplexfold=lambda a, b: types.SimpleNamespace(
            energy=float(__import__("numpy").float32(e) / __import__("numpy").float32(100)), i=i, j=j, structure=st))
        flip = {'(': ')', ')': '(', '.': '.', '&': '&'}
        env = dict(RNA=rna, NucPair=NucPair, scramble=lambda *a: [], cofold_energies=lambda *a: [0.0, 0.0],
                   pvalue_function=lambda *a: 0.0, zscore_function=lambda *a: z,
                   flip_structure=lambda s: ''.join(flip[c] for c in s[::-1]),
                   cur_record=types.SimpleNamespace(seq="N" * 100000), print=lambda *a, **k: None)
        exec(code, env)
        f, bp = io.StringIO(), {}
        env["per_pair"](frag, dup, jw, kw, jw, -25, 100, "mono", [], bp, f, 1)
        pairs = [list(x.v) for key in bp for x in bp[key]]
        out.append(dict(name=name, frag=frag, dup_frag=dup, j_win=jw, k_win=kw, energy_dcal=e, i=i, j=j, structure=st,
                        cofold_zscore=z, row=f.getvalue(), pairs=pairs))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lri_cases.json"), "w") as w:
        json.dump(out, w, indent=1)
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main(sys.argv[1])

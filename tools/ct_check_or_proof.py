#!/usr/bin/env python3
"""Constant-time evidence for zkp_or_prove (zkp_or_mi355x.h), by the recipe of tools/ct_check_transcript_rng.py: the DLEQ disjunction of
tests/or_proof_cases.py (S2) at k = 3 over 257 proofs runs once per class of secret input -- `real` all 0, all k - 1, j mod k, random; the
witness all 0, all l - 1, random -- with rocprofv3 counting the executed instructions and the LDS bank conflicts of every dispatch: counters
only, no tracing in the same run; the instruction counters and the LDS counters in two runs of their own.  Everything else -- the points,
the transcripts, the entropy, k, N -- is equal across the classes (the points are random valid points: a proof need not verify to be timed).
Equal counters across the classes: no branch was taken or skipped, no load or store issued and no LDS cycle spent because of the secret
branch or the witness.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o orp -- python tools/ct_check_or_proof.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o orp -- python tools/ct_check_or_proof.py
    python tools/ct_check_or_proof.py --summarise OUT_A/.../orp_counter_collection.csv OUT_B/.../orp_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

K, N = 3, 257
L = 2**252 + 27742317777372353535851937790883648493
REAL_CLASSES = ["all 0", "all k - 1", "j mod k", "random"]
WITNESS_CLASSES = ["all 0", "all l - 1", "random"]
WATCHED = ("k_or_assemble", "k_or_respond", "k_or_witness", "k_strobe_witness_rng", "k_terms", "k_or_challenge")


def run():
    from tests import or_proof_cases as C
    from zkp_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(11)
    c, fst = C.Case("S2", K, N), C.fused_statement("S2")
    j = np.arange(N)
    reals = {"all 0": np.zeros(N, np.uint8), "all k - 1": np.full(N, K - 1, np.uint8), "j mod k": (j % K).astype(np.uint8),
             "random": rng.integers(0, K, size=N).astype(np.uint8)}
    wits = {"all 0": np.zeros((N, 1, 32), np.uint8), "all l - 1": np.tile(np.frombuffer((L - 1).to_bytes(32, "little"), np.uint8), (N, 1, 1)),
            "random": c.secrets}
    for w in WITNESS_CLASSES:                            # one call per class, witness class by witness class, real class by real class
        for r in REAL_CLASSES:
            eng.or_prove(fst, c.transcripts.copy(), wits[w], reals[r], c.inst, c.common, c.entropy)
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zkp::", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    calls = len(REAL_CLASSES) * len(WITNESS_CLASSES)
    print("# zkp_or_prove, statement S2 (DLEQ) at k = %d over %d proofs; one call per (witness class, real class): witness %s x real %s, listed witness "
          "class by witness class; points, transcripts and entropy equal across the calls" % (K, N, WITNESS_CLASSES, REAL_CLASSES))
    ok = True
    seen = set()
    for k in sorted(per):
        watched = [w for w in WATCHED if k.startswith(w)]
        if not watched:
            continue
        seen.update(watched)
        for c, v in sorted(per[k].items()):
            per_call = len(v) // calls if len(v) % calls == 0 else 0             # a kernel launched several times per call: compare launch by launch
            same = per_call > 0 and all(v[i] == v[i % per_call] for i in range(len(v)))
            ok &= same
            print("%-44s %-22s %s  %s" % (k[:44], c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
    ok &= seen == set(WATCHED)
    print("# verdict:", "every counter of the watched kernels identical across the classes of real and witness" if ok else
          "counters differ or a kernel is missing (seen: %s)" % sorted(seen))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

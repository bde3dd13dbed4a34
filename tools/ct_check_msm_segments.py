#!/usr/bin/env python3
"""Constant-time evidence for zkp_msm_segments with ZKP_CT (zkp_mi355x.h (11)), by the recipe of tools/ct_check_point_mul.py: ONE job -- 16
segments of 4,096 terms over 4,096 shared points, so the classified term path with comb tables and a three-level fold -- run over five very
different scalar classes, with rocprofv3 counting the executed instructions and the LDS bank conflicts of every dispatch: counters only, no
tracing in the same run; the instruction counters and the LDS counters in two runs of their own.  Equal counters across the classes, for the term
kernels and for every kernel of the fold: no branch was taken or skipped, no load or store issued and no crossbar / LDS cycle spent because of
a scalar.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o ms -- python tools/ct_check_msm_segments.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o ms -- python tools/ct_check_msm_segments.py
    python tools/ct_check_msm_segments.py --summarise OUT_A/.../ms_counter_collection.csv OUT_B/.../ms_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_SEG, LENGTH = 16, 4096
L = 2**252 + 27742317777372353535851937790883648493
SCALARS = ["zero", "one", "l-1", "2^256-1", "random"]
WATCHED = ("k_terms_", "k_sum_fold_parts", "k_sum_fold<false>", "k_sum_encode")       # kernel name prefixes: the term kernels and the fold


def scalars(kind, rng, n):
    fixed = {"zero": 0, "one": 1, "l-1": L - 1, "2^256-1": 2**256 - 1}
    if kind in fixed:
        return np.tile(np.frombuffer(fixed[kind].to_bytes(32, "little"), np.uint8), (n, 1))
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def run():
    from zkp_amd.engine import Engine, ZKP_CT
    eng = Engine(0)
    rng = np.random.default_rng(8)
    pts = eng.mul_base(rng.integers(0, 256, size=(LENGTH, 32), dtype=np.uint8))
    t = N_SEG * LENGTH
    off = np.arange(0, t + 1, LENGTH, dtype=np.uint32)
    pidx = np.tile(np.arange(LENGTH, dtype=np.uint32), N_SEG)
    for kind in SCALARS:                            # one call per scalar class, in this order: every kernel of the call is dispatched once per class
        out, st = eng.msm_segments(off, scalars(kind, rng, t), pts, pidx, ZKP_CT)
        assert not st.any()
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zkp::", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# zkp_msm_segments, ZKP_CT, %d segments of %d terms over %d shared points; one call per scalar class (%s); a kernel launched k times per"
          " call lists its k dispatches class by class" % (N_SEG, LENGTH, LENGTH, ", ".join(SCALARS)))
    ok = True
    seen = set()
    for k in sorted(per):
        watched = [w for w in WATCHED if k.startswith(w)]
        if not watched:
            continue
        seen.update(watched)
        for c, v in sorted(per[k].items()):
            per_call = len(v) // len(SCALARS)
            same = per_call > 0 and len(v) == per_call * len(SCALARS) and all(v[i] == v[i % per_call] for i in range(len(v)))
            ok &= same
            print("%-44s %-22s %s  %s" % (k[:44], c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
    print("# the other kernels of the run read no scalar (set-up, decode, classification, tables, copies) and are not compared: "
          + ", ".join(k for k in sorted(per) if not any(k.startswith(w) for w in WATCHED)))
    ok &= seen == set(WATCHED)
    print("# verdict:", "every counter of the term kernels and of the fold identical across the scalar classes" if ok else "counters differ or a kernel is missing")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

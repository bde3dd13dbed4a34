#!/usr/bin/env python3
"""Constant-time evidence for zkp_sc_reduce (zkp_mi355x.h (12)), by the recipe of tools/ct_check_msm_segments.py: ONE ragged job per op -- empty
segments, short ones, segments that cross group edges and one of 40,000 terms, 45,130 terms in all, so a three-level fold -- run over five very
different scalar classes, with rocprofv3 counting the executed instructions and the LDS bank conflicts of every dispatch: counters only, no tracing
in the same run; the instruction counters and the LDS counters in two runs of their own.  Equal counters across the classes for every fold kernel:
no branch was taken or skipped, no load or store issued and no LDS cycle spent because of a scalar.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o sr -- python tools/ct_check_scalar_reduce.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o sr -- python tools/ct_check_scalar_reduce.py
    python tools/ct_check_scalar_reduce.py --summarise OUT_A/.../sr_counter_collection.csv OUT_B/.../sr_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

LENS = [0, 1, 300, 40000, 7, 0, 2000, 255, 257, 2, 2, 2, 2304, 0]
L = 2**252 + 27742317777372353535851937790883648493
SCALARS = ["zero", "one", "l-1", "2^256-1", "random"]
OPS = 3
WATCHED = ("k_sc_fold<",)


def scalars(kind, rng, n):
    fixed = {"zero": 0, "one": 1, "l-1": L - 1, "2^256-1": 2**256 - 1}
    if kind in fixed:
        return np.tile(np.frombuffer(fixed[kind].to_bytes(32, "little"), np.uint8), (n, 1))
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def run():
    from zkp_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(8)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint32)
    t = int(off[-1])
    assert eng._lib.zkp_sc_reduce_levels(t) == 3
    for op in range(OPS):                               # per op one call per scalar class, in this order: every level is dispatched once per call
        for kind in SCALARS:
            a = scalars(kind, rng, t)
            eng.scalar_reduce(op, off, a, None, scalars(kind, rng, t) if op == 2 else None)
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zkp::", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# zkp_sc_reduce, ops SUM, PRODUCT, DOT; segments of %s terms; per op one call per scalar class (%s); a kernel launched k times per class lists"
          " its dispatches class by class" % (LENS, ", ".join(SCALARS)))
    ok = True
    seen = set()
    for k in sorted(per):
        watched = [w for w in WATCHED if k.startswith(w)]
        if not watched:
            continue
        seen.update(watched)
        for c, v in sorted(per[k].items()):
            n_classes = len(SCALARS)
            # the same kernel (k_sc_fold<0, false> serves the later levels of SUM and DOT) may be dispatched for several ops: the dispatches of one op
            # come class by class, per_call of them per class, so the sequence must repeat with the period per_call inside each block of an op
            per_op = len(v) // n_classes if len(v) % n_classes == 0 else 0
            same = per_op > 0 and _periodic(v, n_classes)
            ok &= same
            print("%-44s %-22s %s  %s" % (k[:44], c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
    print("# the other kernels of the run read no scalar and are not compared: " + ", ".join(k for k in sorted(per) if not any(k.startswith(w) for w in WATCHED)))
    ok &= seen == set(WATCHED)
    print("# verdict:", "every counter of every fold kernel identical across the scalar classes" if ok else "counters differ or a kernel is missing")


def _periodic(v, n_classes):
    """v = blocks (one per op that dispatches the kernel) of n_classes equal groups: true when every block repeats its first group n_classes times"""
    for ops in (1, 2, 3):
        if len(v) % (ops * n_classes):
            continue
        per_call = len(v) // (ops * n_classes)
        block = per_call * n_classes
        if all(v[i] == v[(i // block) * block + i % per_call] for i in range(len(v))):
            return True
    return False


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

#!/usr/bin/env python3
"""Constant-time evidence for the batched scalar kernels (k_sc_invert, k_sc_muladd, k_sc_from_wide), by the recipe of tools/ct_check.py:
the same call at n = 65,536 over very different operands, with rocprofv3 counting the executed instructions of every dispatch.  Equal
counters across the inputs: no branch was taken or skipped and no load or store issued because of an operand.

    rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAVES \\
              --output-format csv -d OUT -o sc -- python tools/ct_check_scalars.py
    python tools/ct_check_scalars.py --summarise OUT/sc_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N = 65536
L = 2**252 + 27742317777372353535851937790883648493
PATTERNS = ["zero", "one", "l-1", "2^256-1", "one random scalar for all", "random-a", "random-b"]
KERNELS = ("k_sc_invert", "k_sc_muladd", "k_sc_from_wide")


def operand(kind, rng, width=32):
    fixed = {"zero": 0, "one": 1, "l-1": L - 1, "2^256-1": 2**256 - 1}
    if kind in fixed:
        v = fixed[kind] if width == 32 else fixed[kind] | (fixed[kind] << 256)
        return np.tile(np.frombuffer(v.to_bytes(width, "little"), np.uint8), (N, 1))
    if kind == "one random scalar for all":
        return np.tile(rng.integers(0, 256, size=(1, width), dtype=np.uint8), (N, 1))
    return rng.integers(0, 256, size=(N, width), dtype=np.uint8)


def run():
    from zkp_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(7)
    for kind in PATTERNS:                       # one dispatch of each kernel per pattern, in this order
        a = operand(kind, rng)
        eng.scalar_invert(a)
        eng.scalar_muladd(a, operand(kind, rng), operand(kind, rng))
        eng.scalar_from_wide(operand(kind, rng, 64))
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# n = %d; one dispatch per operand pattern: %s" % (N, ", ".join(PATTERNS)))
    ok = True
    for k in KERNELS:
        for c, v in sorted(per[k].items()):
            same = len(v) == len(PATTERNS) and len(set(v)) == 1
            ok &= same
            print("%-16s %-18s %s  %s" % (k, c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
        ok &= bool(per[k])
    print("# verdict:", "every counter identical across operand patterns, per kernel" if ok else "counters differ or a kernel is missing")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

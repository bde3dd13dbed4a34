#!/usr/bin/env python3
"""Constant-time evidence for zkp_sc_scan (zkp_mi355x.h (13)), by the recipe of tools/ct_check_scalar_reduce.py: ONE ragged job -- empty segments,
short ones, segments that cross unit edges and one of 60,000 terms, 67,130 terms in all, so a three-level plan of five launches -- run per op and
mode over five very different scalar classes, with rocprofv3 counting the executed instructions and the LDS bank conflicts of every dispatch:
counters only, no tracing in the same run; the instruction counters and the LDS counters in two runs of their own.  Equal counters across the
classes for every scan kernel: no branch was taken or skipped, no load or store issued and no LDS cycle spent because of a scalar.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o ss -- python tools/ct_check_scalar_scan.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o ss -- python tools/ct_check_scalar_scan.py
    python tools/ct_check_scalar_scan.py --summarise OUT_A/.../ss_counter_collection.csv OUT_B/.../ss_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

LENS = [0, 1, 300, 60000, 7, 0, 2000, 255, 257, 2, 2, 2, 4304, 0]
L = 2**252 + 27742317777372353535851937790883648493
SCALARS = ["zero", "one", "l-1", "2^256-1", "random"]
OPS = 2
MODES = 2
WATCHED = ("k_sc_scan<",)


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
    assert eng._lib.zkp_sc_scan_launches(t) == 5
    for op in range(OPS):                               # per op and mode one call per scalar class, in this order
        for mode in range(MODES):
            for kind in SCALARS:
                eng.scalar_scan(op, off, scalars(kind, rng, t), None, bool(mode))
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zkp::", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# zkp_sc_scan, ops SUM, PRODUCT, modes inclusive, exclusive; segments of %s terms; per op and mode one call per scalar class (%s); a kernel"
          " launched k times per call lists its dispatches mode by mode, class by class" % (LENS, ", ".join(SCALARS)))
    ok = True
    seen = set()
    for k in sorted(per):
        watched = [w for w in WATCHED if k.startswith(w)]
        if not watched:
            continue
        seen.update(watched)
        for c, v in sorted(per[k].items()):
            same = _periodic(v, len(SCALARS))
            ok &= same
            print("%-44s %-22s %s  %s" % (k[:44], c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
    print("# the other kernels of the run read no scalar and are not compared: " + ", ".join(k for k in sorted(per) if not any(k.startswith(w) for w in WATCHED)))
    ok &= seen == set(WATCHED)
    print("# verdict:", "every counter of every scan kernel identical across the scalar classes" if ok else "counters differ or a kernel is missing")


def _periodic(v, n_classes):
    """v = MODES blocks of n_classes equal groups (a kernel's dispatches of one call): true when every block repeats its first group n_classes times"""
    if len(v) == 0 or len(v) % (MODES * n_classes):
        return False
    per_call = len(v) // (MODES * n_classes)
    block = per_call * n_classes
    return all(v[i] == v[(i // block) * block + i % per_call] for i in range(len(v)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

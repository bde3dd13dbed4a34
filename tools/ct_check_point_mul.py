#!/usr/bin/env python3
"""Constant-time evidence for k_mul_base and k_mul_pairs<true> (zkp_mi355x.h (8)), by the recipe of tools/ct_check_scalars.py: the same call
at n = 65,536 over very different operands, with rocprofv3 counting the executed instructions and the LDS bank conflicts of every
dispatch -- counters only, no tracing in the same run; the instruction counters and the LDS counters in two runs of their own.  Equal counters across the operand patterns: no branch was taken or skipped, no load
or store issued and no crossbar / LDS cycle spent because of a scalar -- or, for k_mul_pairs<true>, because a point did or did not decode.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o pm -- python tools/ct_check_point_mul.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o pm -- python tools/ct_check_point_mul.py
    python tools/ct_check_point_mul.py --summarise OUT_A/.../pm_counter_collection.csv OUT_B/.../pm_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N = 65536
L = 2**252 + 27742317777372353535851937790883648493
SCALARS = ["zero", "one", "l-1", "2^256-1", "random"]
POINTS = ["valid", "invalid"]
KERNELS = {"k_mul_base": len(SCALARS), "k_mul_pairs<true>": len(SCALARS) * len(POINTS)}
# RFC 9496 appendix A.3: a non-canonical field element, a negative s, a non-square
INVALID = ["edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f", "0100000000000000000000000000000000000000000000000000000000000000",
           "26948d35ca62e643e26a83177332e6b6afeb9d08e4268b650f1f5bbd8d81d371"]


def scalars(kind, rng):
    fixed = {"zero": 0, "one": 1, "l-1": L - 1, "2^256-1": 2**256 - 1}
    if kind in fixed:
        return np.tile(np.frombuffer(fixed[kind].to_bytes(32, "little"), np.uint8), (N, 1))
    return rng.integers(0, 256, size=(N, 32), dtype=np.uint8)


def run():
    from zkp_amd.engine import Engine, ZKP_CT
    eng = Engine(0)
    rng = np.random.default_rng(8)
    valid = eng.mul_base(rng.integers(0, 256, size=(N, 32), dtype=np.uint8))      # (one more k_mul_base dispatch, the first: skipped by the summary)
    invalid = np.frombuffer(b"".join(bytes.fromhex(INVALID[i % len(INVALID)]) for i in range(N)), np.uint8).reshape(N, 32)
    for kind in SCALARS:                            # one dispatch of k_mul_base and two of k_mul_pairs<true> per scalar pattern, in this order
        s = scalars(kind, rng)
        eng.mul_base(s)
        for pts in (valid, invalid):
            out, st = eng.mul_points(s, pts, ZKP_CT)
            assert st.all() == (pts is invalid) and st.any() == (pts is invalid)
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# n = %d; k_mul_base: one dispatch per scalar pattern (%s); k_mul_pairs<true>: per scalar pattern one dispatch over valid points and one over"
          " encodings that do not decode" % (N, ", ".join(SCALARS)))
    ok = True
    for k, want in KERNELS.items():
        for c, v in sorted(per[k].items()):
            if k == "k_mul_base":
                v = v[1:]                                                      # (the dispatch that made the valid points)
            same = len(v) == want and len(set(v)) == 1
            ok &= same
            print("%-18s %-22s %s  %s" % (k, c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
        ok &= bool(per[k])
    print("# verdict:", "every counter identical across operand patterns, per kernel" if ok else "counters differ or a kernel is missing")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()

#!/usr/bin/env python3
"""Hash to the group (RFC 9496 section 4.3.4, zkp_mi355x.h (5)) on one MI355X: what the batched map and the VRF example's
`hash_to_group` cost.

    python tools/hash_to_group_bench.py              # outputs/s of k_from_uniform (HIP events) at n = 4096, 65,536, 2^20; the
                                                     # zkp_hash_to_group_batch call at N = 4096 on both transcript routes; the host
                                                     # backend on one thread
    rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR --output-format csv -d OUT -o ct \\
              -- python tools/hash_to_group_bench.py --ct
    python tools/hash_to_group_bench.py --summarise OUT/ct_counter_collection.csv

--ct runs k_from_uniform once per input set (zeros, 0xff, random, inputs whose two Elligator maps both take the non-square branch), all of
the same size, nothing else; --summarise checks that the instruction counters are identical across the sets (constant-time evidence in
the style of tools/ct_check.py)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CT_SETS = ("zeros", "0xff", "random", "non-square")
CT_N = 16384
P = 2**255 - 19


def _non_square_halves(k, rng):
    """k random 32-byte halves whose Elligator map takes the was_square = 0 branch (RFC 9496 4.3.4), by the field's own arithmetic"""
    d = (-121665 * pow(121666, P - 2, P)) % P
    i = pow(2, (P - 1) // 4, P)
    out = []
    while len(out) < k:
        h = rng.bytes(32)
        t = (int.from_bytes(h, "little") & ((1 << 255) - 1)) % P
        r = i * t * t % P
        u = (r + 1) * (1 - d * d) % P
        v = (-1 - r * d) * (r + d) % P
        x = u * pow(v, P - 2, P) % P                                   # u / v is a square iff x^((p-1)/2) is 0 or 1
        if x and pow(x, (P - 1) // 2, P) != 1:
            out.append(h)
    return b"".join(out)


def ct_inputs(kind, n, rng):
    if kind == "zeros":
        return np.zeros((n, 64), np.uint8)
    if kind == "0xff":
        return np.full((n, 64), 0xff, np.uint8)
    if kind == "random":
        return rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    return np.frombuffer(_non_square_halves(2 * n, rng), np.uint8).reshape(n, 64).copy()


def ct_run():
    from zkp_amd.engine import Engine
    rng = np.random.default_rng(9496)
    sets = [ct_inputs(k, CT_N, rng) for k in CT_SETS]                # all inputs first: the profiled process launches nothing else in between
    eng = Engine(0)
    for k, rows in zip(CT_SETS, sets):
        eng.from_uniform_bytes(rows)
        print("ran k_from_uniform on %d outputs: %s" % (CT_N, k))
    eng.close()


def summarise(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "k_from_uniform" in r.get("Kernel_Name", "")]
    by = {}
    for r in rows:
        by.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = by.get(int(r["Dispatch_Id"]), {}).get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    ids = sorted(by)
    assert len(ids) == len(CT_SETS), "expected %d dispatches of k_from_uniform, found %d" % (len(CT_SETS), len(ids))
    names = sorted(by[ids[0]])
    print("# k_from_uniform, %d outputs per dispatch, one dispatch per input set (rocprofv3 --pmc, counters summed over the dispatch)" % CT_N)
    print("%-12s " % "input set" + " ".join("%18s" % n for n in names))
    for k, i in zip(CT_SETS, ids):
        print("%-12s " % k + " ".join("%18.0f" % by[i][n] for n in names))
    same = all(by[i] == by[ids[0]] for i in ids)
    print("# verdict:", "every counter is identical across the input sets: no branch taken or skipped and no load or store made or "
          "skipped because of the input" if same else "COUNTERS DIFFER between input sets")
    return same


def bench():
    from zkp_amd.engine import Engine
    from zkp_amd import toolbox as T
    rng = np.random.default_rng(1)
    eng = Engine(0)
    reps = 20
    print("# k_from_uniform: kernel time from HIP events (zkp_ctx_last_timing, kind decode), median of %d calls; call = the synchronous host-pointer call" % reps)
    for n in (4096, 65536, 1 << 20):
        rows = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        eng.from_uniform_bytes(rows)                                    # warm: workspace, code object
        eng.set_profiling(True)
        ks, calls = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.from_uniform_bytes(rows)
            calls.append(time.perf_counter() - t0)
            ks.append(eng.last_timing()[0]["decode"])
        eng.set_profiling(False)
        k = float(np.median(ks))
        print("n = %8d   kernel %8.3f ms = %6.2f M outputs/s   call %8.3f ms (copies included)" % (n, k, n / k / 1e3, 1e3 * float(np.median(calls))))
    n = 4096
    msgs = [rng.bytes(32) for _ in range(n)]

    def transcripts():
        ts = []
        for m in msgs:
            t = T.Transcript(b"My VRF Application")
            t.append_message(b"msg", m)
            ts.append(t.state)
        return np.stack(ts)

    old_host = T.get_host_max_terms()
    T.set_host_max_terms(0)
    old_fused = T.get_fused_min_batch()
    try:
        for route, fmb in (("device transcripts", 0), ("host transcripts, device map", 0xffffffff)):
            T.set_fused_min_batch(fmb)
            T.hash_to_group(eng, transcripts())
            times = []
            for _ in range(reps):
                ts = transcripts()
                t0 = time.perf_counter()
                T.hash_to_group(eng, ts)
                times.append(time.perf_counter() - t0)
            print("hash_to_group N = %d, %-28s %8.3f ms per call (median)" % (n, route + ":", 1e3 * float(np.median(times))))
    finally:
        T.set_fused_min_batch(old_fused)
        T.set_host_max_terms(old_host)
    rows = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    t0 = time.perf_counter()
    T.from_uniform_bytes(None, rows, threads=1)
    dt = time.perf_counter() - t0
    print("host backend, 1 thread: n = %d in %.1f ms = %.1f us per output" % (n, 1e3 * dt, 1e6 * dt / n))
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        sys.exit(0 if summarise(sys.argv[2]) else 1)
    elif len(sys.argv) > 1 and sys.argv[1] == "--ct":
        ct_run()
    else:
        bench()

#!/usr/bin/env python3
"""Batched point sums (zkp_mi355x.h (9)) on one MI355X against the route callers had before -- Engine.msm_many on the equivalent CSR job with
scalars 1 and l - 1, ZKP_VARTIME -- both routes in one process.

    python tools/point_sum_bench.py [max_terms]

Shapes: pairs (zkp_add_points) and sums of two terms (zkp_sum_points) at 4,096, 65,536 and 2^20 outputs; sums of 1,024 terms at 64 and 1,024
outputs; one sum of 65,536 terms and one of 2^20.  Every term is a distinct point.

Per call and shape: `stream` = the time between HIP events around everything the call queues on its stream (zkp_ctx_last_timing's total: every
kernel of the call and the gaps between them, no copies), `call` = the synchronous host-pointer call, copies included.  Each shape is warmed up,
then the routes alternate, REPS rounds; min / median / max over the rounds are printed (the spread is the margin of the comparison).  The host
backend at 16 threads is measured for 65,536 pairs."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

L = 2**252 + 27742317777372353535851937790883648493


def measure(routes, reps):
    """routes = [(name, engine, call)] -> {name: (stream ms [reps], call ms [reps])}, the routes taken in turn inside every round"""
    for _, eng, f in routes:                                            # warm: workspace, code objects
        f()
        f()
    res = {name: ([], []) for name, _, _ in routes}
    for _ in range(reps):
        for name, eng, f in routes:
            eng.set_profiling(True)
            f()
            res[name][0].append(eng.last_timing()[1])
            eng.set_profiling(False)
            t0 = time.perf_counter()
            f()
            res[name][1].append(1e3 * (time.perf_counter() - t0))
    return res


def spread(v):
    return "%9.3f / %9.3f / %9.3f" % (min(v), float(np.median(v)), max(v))


def report(what, n_out, n_terms, routes, res):
    new = routes[0][0]
    for name, _, _ in routes:
        k, c = res[name]
        print("%-22s outputs = %8d terms = %8d  %-28s stream min/med/max %s ms  call %s ms  = %9.2f M terms/s (stream median)"
              % (what, n_out, n_terms, name, spread(k), spread(c), n_terms / float(np.median(k)) / 1e3))
    for name, _, _ in routes[1:]:
        for which, col in (("stream", 0), ("call", 1)):
            a, b = res[new][col], res[name][col]
            verdict = "faster beyond the spread" if max(a) < min(b) else ("faster by the medians, spreads overlap" if np.median(a) < np.median(b) else "NOT faster")
            print("%-22s outputs = %8d  %s against %s, %s: x %.2f (medians) -- %s" % (what, n_out, new, name, which, float(np.median(b)) / float(np.median(a)), verdict))


def kernels(tag, eng, f):
    eng.set_profiling(True)
    f()
    print("#   %s kernels:" % tag, eng.last_kernels(), {k: round(v, 3) for k, v in eng.last_timing()[0].items() if v})
    eng.set_profiling(False)


def main():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine, ZKP_PT_ADD, ZKP_VARTIME
    max_terms = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 21
    rng = np.random.default_rng(99)
    e_new, e_old = Engine(0), Engine(0)
    print("# one MI355X; stream = HIP events around the call's stream work; call = synchronous host-pointer call; min / median / max over the rounds")
    print("# zkp_sum_points_group() =", e_new._lib.zkp_sum_points_group())
    n_max = min(max_terms, 1 << 21)
    pts = e_new.mul_base(rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8))         # distinct points
    one = np.frombuffer((1).to_bytes(32, "little"), np.uint8)
    ones = np.ascontiguousarray(np.tile(one, (n_max, 1)))

    def old(off, t):
        return lambda: e_old.msm_many(off, ones[:t], np.arange(t, dtype=np.uint32), pts[:t], ZKP_VARTIME)

    for n in (4096, 65536, 1 << 20):
        if 2 * n > n_max:
            continue
        reps = 15 if n <= 4096 else (9 if n <= 65536 else 5)
        off = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
        a, b = np.ascontiguousarray(pts[0:2 * n:2]), np.ascontiguousarray(pts[1:2 * n:2])
        f_pairs = lambda: e_new.add_points(a, b, ZKP_PT_ADD)
        f_sums = lambda: e_new.sum_points(off, pts[:2 * n])
        routes = [("add_points (k_add_pairs)", e_new, f_pairs), ("msm_many, scalars 1", e_old, old(off, 2 * n))]
        report("pairs", n, 2 * n, routes, measure(routes, reps))
        kernels("add_points", e_new, f_pairs)
        routes = [("sum_points (fold)", e_new, f_sums), ("msm_many, scalars 1", e_old, old(off, 2 * n))]
        report("sums of 2 terms", n, 2 * n, routes, measure(routes, reps))
        kernels("sum_points", e_new, f_sums)
        kernels("msm_many", e_old, old(off, 2 * n))
        if n == 65536:
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                T.point_add(None, a, b, threads=16)
                ts.append(1e3 * (time.perf_counter() - t0))
            print("host backend           outputs = %8d  point_add, 16 threads  min/med/max %s ms = %7.3f M outputs/s" % (n, spread(ts), n / float(np.median(ts)) / 1e3))
    for n_out, length in ((64, 1024), (1024, 1024), (1, 65536), (1, 1 << 20)):
        t = n_out * length
        if t > n_max:
            continue
        reps = 7 if t <= 65536 else 3
        off = np.arange(0, t + 1, length, dtype=np.uint32)
        f_sums = lambda: e_new.sum_points(off, pts[:t])
        routes = [("sum_points (fold)", e_new, f_sums), ("msm_many, scalars 1", e_old, old(off, t))]
        report("sums of %d terms" % length, n_out, t, routes, measure(routes, reps))
        kernels("sum_points", e_new, f_sums)
        kernels("msm_many", e_old, old(off, t))
    for e in (e_new, e_old):
        e.close()


if __name__ == "__main__":
    main()

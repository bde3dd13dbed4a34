#!/usr/bin/env python3
"""Batched Scalar * basepoint and Scalar * point (zkp_mi355x.h (8)) on one MI355X against the route callers had before -- Engine.msm_many on
the CSR job off = arange(n + 1), pidx = arange(n) -- for n = 4,096, 65,536, 262,144 and 2^20, both routes in one process.

    python tools/point_mul_bench.py [max_n]

Per call and size: `stream` = the time between HIP events around everything the call queues on its stream (zkp_ctx_last_timing's total:
every kernel of the call and the gaps between them, no copies), `call` = the synchronous host-pointer call, copies included.  Each shape is
warmed up, then the routes alternate, REPS rounds; min / median / max over the rounds are printed (the spread is the margin of the
comparison).  For the basepoint the old route is measured twice, in contexts of their own: B unregistered, and after zkp_ctx_prepare_fixed_points([B]).
The host backend at 16 threads is measured at 65,536."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SIZES = (4096, 65536, 262144, 1 << 20)
REPS = {4096: 15, 65536: 9, 262144: 7, 1 << 20: 5}
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


def measure(routes, reps):
    """routes = [(name, engine, call)] -> {name: (stream ms [reps], call ms [reps])}, the routes taken in turn inside every round"""
    for _, eng, f in routes:                                            # warm: workspace, tables, code objects
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


def report(what, n, routes, res, eng_new):
    new = routes[0][0]
    for name, _, _ in routes:
        k, c = res[name]
        print("%-12s n = %8d  %-34s stream min/med/max %s ms  call %s ms  = %8.2f M outputs/s (stream median)"
              % (what, n, name, spread(k), spread(c), n / float(np.median(k)) / 1e3))
    for name, _, _ in routes[1:]:
        a, b = res[new][0], res[name][0]
        verdict = "faster beyond the spread" if max(a) < min(b) else ("faster by the medians, spreads overlap" if np.median(a) < np.median(b) else "NOT faster")
        print("%-12s n = %8d  %s against %s: x %.2f (medians) -- %s" % (what, n, new, name, float(np.median(b)) / float(np.median(a)), verdict))


def main():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine, ZKP_CT, ZKP_VARTIME
    max_n = int(sys.argv[1]) if len(sys.argv) > 1 else max(SIZES)
    rng = np.random.default_rng(255)
    e_new, e_old, e_reg = Engine(0), Engine(0), Engine(0)
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    e_reg.prepare_fixed_points(B)
    print("# one MI355X; stream = HIP events around the call's stream work; call = synchronous host-pointer call; min / median / max over the rounds")
    for n in [s for s in SIZES if s <= max_n]:
        sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        off, pidx, zeros = np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)
        pts = e_new.mul_base(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))            # n distinct points
        routes = [("mul_base (k_mul_base)", e_new, lambda: e_new.mul_base(sc)),
                  ("msm_many CT, B unregistered", e_old, lambda: e_old.msm_many(off, sc, zeros, B, ZKP_CT)),
                  ("msm_many CT, B registered", e_reg, lambda: e_reg.msm_many(off, sc, zeros, B, ZKP_CT))]
        res = measure(routes, REPS[n])
        report("basepoint", n, routes, res, e_new)
        e_new.set_profiling(True)
        e_new.mul_base(sc)
        print("#   kernels:", e_new.last_kernels(), {k: round(v, 3) for k, v in e_new.last_timing()[0].items() if v})
        e_new.set_profiling(False)
        for flags, tag in ((ZKP_CT, "CT"), (ZKP_VARTIME, "VARTIME")):
            routes = [("mul_points %s (k_mul_pairs)" % tag, e_new, lambda f=flags: e_new.mul_points(sc, pts, f)),
                      ("msm_many %s, arange indices" % tag, e_old, lambda f=flags: e_old.msm_many(off, sc, pidx, pts, f))]
            res = measure(routes, REPS[n])
            report("points " + tag, n, routes, res, e_new)
            for k, e in enumerate((e_new, e_old)):
                e.set_profiling(True)
                routes[k][2]()
                print("#   kernels:", e.last_kernels(), {k: round(v, 3) for k, v in e.last_timing()[0].items() if v})
                e.set_profiling(False)
        if n == 65536:
            for name, f in (("basepoint_mul", lambda: T.basepoint_mul(None, sc, threads=16)), ("point_mul CT", lambda: T.point_mul(None, sc, pts, ZKP_CT, threads=16)),
                            ("point_mul VARTIME", lambda: T.point_mul(None, sc, pts, ZKP_VARTIME, threads=16))):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    f()
                    ts.append(1e3 * (time.perf_counter() - t0))
                print("host backend n = %8d  %-20s 16 threads  min/med/max %s ms = %7.3f M outputs/s" % (n, name, spread(ts), n / float(np.median(ts)) / 1e3))
    for e in (e_new, e_old, e_reg):
        e.close()


if __name__ == "__main__":
    main()

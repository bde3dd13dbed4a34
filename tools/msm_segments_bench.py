#!/usr/bin/env python3
"""Multiscalar sums with long segments (zkp_mi355x.h (11)) on one MI355X against the route callers had before -- Engine.msm_many on the same
job, whose code is unchanged -- both routes in one process, in constant and in variable time.

    python tools/msm_segments_bench.py [long] [short] [optional] [--out FILE]

    long      64 x 1,024, 1,024 x 1,024, 1 x 65,536 and 1 x 2^20 terms with a point per term, 16 x 65,536 over 65,536 shared points
    short     4,096 and 65,536 MSMs of 2, 11, 32 and 128 terms, a point per term: where zkp_msm_many's shared-inversion encoder is expected to win,
              and what the default of zkp_toolbox_get_msm_fold_min_segment() is read from
    optional  one variable-time MSM of 65,536 and of 2^20 terms with a point per term against Engine.msm_optional (the bucket method)

Without a part all three run.  Scalars are random 256-bit values.  Per call and shape: `stream` = the time between HIP events around everything
the call queues on its stream (zkp_ctx_last_timing's total: every kernel of the call and the gaps between them, no copies), `call` = the
synchronous host-pointer call, copies included.  Each shape is warmed up, then the routes alternate; min / median / max over the rounds are
printed (the spread is the margin of the comparison), then the per-kind split of one call of each route with the kernels it launched.  The
report goes to stdout and, with --out, to the end of FILE as well."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

_out = None


def say(line):
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


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


def report(what, routes, res):
    new = routes[0][0]
    for name, _, _ in routes:
        k, c = res[name]
        say("%-34s %-30s stream min/med/max %s ms  call %s ms" % (what, name, spread(k), spread(c)))
    for name, _, _ in routes[1:]:
        for which, col in (("stream", 0), ("call", 1)):
            a, b = res[new][col], res[name][col]
            verdict = "faster beyond the spread" if max(a) < min(b) else ("faster by the medians, spreads overlap" if np.median(a) < np.median(b) else "NOT faster")
            say("%-34s %s against %s, %s: x %.2f (medians) -- %s" % (what, new, name, which, float(np.median(b)) / float(np.median(a)), verdict))


def kernels(tag, eng, f):
    eng.set_profiling(True)
    f()
    say("#   %s: %s %s" % (tag, {k: round(v, 3) for k, v in eng.last_timing()[0].items() if v}, eng.last_kernels()))
    eng.set_profiling(False)


def main():
    global _out
    from zkp_amd.engine import Engine, ZKP_CT, ZKP_VARTIME
    args = sys.argv[1:]
    if "--out" in args:
        _out = open(args[args.index("--out") + 1], "a")
        del args[args.index("--out"):args.index("--out") + 2]
    parts = args or ["long", "short", "optional"]
    rng = np.random.default_rng(99)
    e_new, e_old = Engine(0), Engine(0)
    say("# one MI355X; parts: %s; stream = HIP events around the call's stream work; call = synchronous host-pointer call; min / median / max over the rounds"
        % " ".join(parts))
    say("# zkp_sum_points_group() = %d" % e_new._lib.zkp_sum_points_group())
    n_max = (1 << 23) if "short" in parts else (1 << 20)
    pts = e_new.mul_base(rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8))         # distinct points
    sc = rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8)
    iota = np.arange(n_max, dtype=np.uint32)
    names = {ZKP_CT: "ct", ZKP_VARTIME: "vartime"}

    def pair(n_out, length, shared, flags):
        t = n_out * length
        off = np.arange(0, t + 1, length, dtype=np.uint32)
        pidx = np.ascontiguousarray(np.tile(iota[:length], n_out)) if shared else iota[:t]
        p = pts[:length] if shared else pts[:t]
        f_new = lambda: e_new.msm_segments(off, sc[:t], p, pidx if shared else None, flags)
        f_old = lambda: e_old.msm_many(off, sc[:t], pidx, p, flags)
        return f_new, f_old

    shapes = []
    if "long" in parts:
        shapes += [(64, 1024, False), (1024, 1024, False), (1, 65536, False), (1, 1 << 20, False), (16, 65536, True)]
    if "short" in parts:
        shapes += [(n, k, False) for n in (4096, 65536) for k in (2, 11, 32, 128)]
    for n_out, length, shared in shapes:
        t = n_out * length
        for flags in (ZKP_VARTIME, ZKP_CT):
            reps = 3 if t >= (1 << 20) else 7
            f_new, f_old = pair(n_out, length, shared, flags)
            routes = [("msm_segments (fold)", e_new, f_new), ("msm_many", e_old, f_old)]
            what = "%d x %d%s %s" % (n_out, length, " shared points" if shared else "", names[flags])
            report(what, routes, measure(routes, reps))
            kernels("msm_segments", e_new, f_new)
            kernels("msm_many", e_old, f_old)
    if "optional" in parts:
        for t in (65536, 1 << 20):
            f_new, _ = pair(1, t, False, ZKP_VARTIME)
            f_opt = lambda: e_old.msm_optional(sc[:t], pts[:t])
            routes = [("msm_segments (fold)", e_new, f_new), ("msm_optional (buckets)", e_old, f_opt)]
            report("1 x %d vartime, own points" % t, routes, measure(routes, 5))
            kernels("msm_optional", e_old, f_opt)
    for e in (e_new, e_old):
        e.close()
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Many variable-time multiscalar sums with long segments (zkp_mi355x.h (14)) on one MI355X against the routes callers had before, all routes in one
process and alternated inside every round.

    python tools/msm_optional_many_bench.py [shapes] [pad] [few] [cap] [--out FILE]

    shapes   point per term: 16 x 65,536, 64 x 16,384, 256 x 4,096, 1,024 x 1,024, 4,096 x 256, one segment of 2^20, a ragged mix of 1,000 segments of
             200 to 2,000 terms and one of 2^18; then 16 x 65,536 over 65,536 shared points.  Routes: zkp_msm_optional_many (the bucket method, many
             segments to a run), zkp_msm_segments with ZKP_VARTIME (a walk per term, then the fold), a loop of zkp_msm_optional_dev per segment on
             resident buffers (up to 1,024 segments), zkp_msm_many for the short shapes.
    pad      what padding costs: the _dev form with every segment padded to its own length and to twice its length
    few      4 and 16 segments of 256, 1,024 and 4,096 terms: few segments of moderate length, where a run is a narrow launch; with the rows of
             `shapes` what the default of zkp_toolbox_get_msm_bucket_min_segment() is read from
    cap      the cap on the padded terms of one run (test-hook build, ZKP_TESTOPT_PIP_RUN_CAP): equal-length jobs of 2^21 terms with the cap at the
             job's size (one run), a half (two) and a quarter (four), and further down: time per term.  The library's cap is the smallest from which
             that time is flat.

Without a part all four run.  Scalars are random 256-bit values.  Per route and shape: `stream` = the time between HIP events around everything the call
queues on its stream (zkp_ctx_last_timing's total: every kernel of the call and the gaps between them, no copies); `call` = the synchronous
host-pointer call, copies included; for the loop of zkp_msm_optional_dev `stream` is the wall time from the first enqueue to the end of
zkp_ctx_synchronize on resident buffers (K launches' worth of gaps belong to that route).  Five rounds; min / median / max are printed -- the spread
is the margin of every comparison.  The report goes to stdout and, with --out, to the end of FILE as well."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROUNDS = 5
_out = None


def say(line):
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


def spread(v):
    return "%9.3f / %9.3f / %9.3f" % (min(v), float(np.median(v)), max(v))


def measure(routes):
    """routes = [(name, stream_ms() -> float or None, call() or None)] -> {name: (stream [ROUNDS], call [ROUNDS])}, routes in turn inside every round"""
    for _, s, c in routes:
        for f in (s, c):
            if f:
                f()
    res = {name: ([], []) for name, _, _ in routes}
    for _ in range(ROUNDS):
        for name, s, c in routes:
            if s:
                res[name][0].append(s())
            if c:
                t0 = time.perf_counter()
                c()
                res[name][1].append(1e3 * (time.perf_counter() - t0))
    return res


def report(what, routes, res, terms):
    new = routes[0][0]
    for name, _, _ in routes:
        k, c = res[name]
        say("%-26s %-30s stream %s ms%s%s" % (what, name, spread(k) if k else "        -", "  call %s ms" % spread(c) if c else "",
                                             "  (%.2f ns per term, stream median)" % (1e6 * float(np.median(k)) / terms) if k and name == new else ""))
    for name, _, _ in routes[1:]:
        for which, col in (("stream", 0), ("call", 1)):
            a, b = res[new][col], res[name][col]
            if not a or not b:
                continue
            verdict = "ahead beyond the spread" if max(a) < min(b) else ("ahead by the medians, spreads overlap" if np.median(a) < np.median(b) else "NOT ahead")
            say("%-26s   %s against %s, %s: x %.2f (medians) -- %s" % (what, new, name, which, float(np.median(b)) / float(np.median(a)), verdict))


def profiled(eng, f):
    def g():
        eng.set_profiling(True)
        f()
        t = eng.last_timing()[1]
        eng.set_profiling(False)
        return t
    return g


def main():
    global _out
    import torch
    from zkp_amd.engine import Engine, ZKP_TESTOPT_PIP_RUN_CAP, ZKP_VARTIME
    args = sys.argv[1:]
    if "--out" in args:
        _out = open(args[args.index("--out") + 1], "a")
        del args[args.index("--out"):args.index("--out") + 2]
    parts = args or ["shapes", "pad", "few", "cap"]
    assert torch.cuda.is_available()
    rng = np.random.default_rng(77)
    e = Engine(0)
    say("# one MI355X; parts: %s; %d rounds, routes alternated in one process; min / median / max" % (" ".join(parts), ROUNDS))
    say("# zkp_msm_optional_many_min_segment() = %d" % e._lib.zkp_msm_optional_many_min_segment())
    n_max = 1 << 21
    pts = e.mul_base(rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8))             # distinct points
    sc = rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8)
    iota = np.arange(n_max, dtype=np.uint32)
    d_sc, d_pts = torch.from_numpy(sc).to("cuda:0"), torch.from_numpy(pts).to("cuda:0")
    d_out = torch.zeros((4096, 32), dtype=torch.uint8, device="cuda:0")
    d_st = torch.zeros((4096,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()

    def loop_dev(off):
        """one zkp_msm_optional_dev per segment on the resident arrays, queued back to back; wall ms to the end of the synchronise"""
        lo = [int(x) for x in off]
        e.synchronize()
        t0 = time.perf_counter()
        for i in range(len(lo) - 1):
            e.msm_optional_dev(lo[i + 1] - lo[i], d_sc.data_ptr() + 32 * lo[i], d_pts.data_ptr() + 32 * lo[i], d_out.data_ptr() + 32 * i, d_st.data_ptr() + 4 * i)
        e.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def shape(what, off, shared_len=0):
        off = np.ascontiguousarray(off, dtype=np.uint32)
        t, n_seg = int(off[-1]), len(off) - 1
        longest = int(np.diff(off.astype(np.int64)).max())
        pidx = np.ascontiguousarray(iota[:t] % shared_len).astype(np.uint32) if shared_len else None
        p = pts[:shared_len] if shared_len else pts[:t]
        f_new = lambda: e.msm_optional_many(off, sc[:t], p, pidx)
        f_seg = lambda: e.msm_segments(off, sc[:t], p, pidx, ZKP_VARTIME)
        routes = [("msm_optional_many (buckets)", profiled(e, f_new), f_new), ("msm_segments vartime (fold)", profiled(e, f_seg), f_seg)]
        if not shared_len and n_seg <= 1024:
            routes.append(("loop of msm_optional_dev", lambda: loop_dev(off), None))
        if longest <= 1024:
            f_many = lambda: e.msm_many(off, sc[:t], iota[:t] if pidx is None else pidx, p, ZKP_VARTIME)
            routes.append(("msm_many vartime", profiled(e, f_many), f_many))
        report(what, routes, measure(routes), t)
        e.set_profiling(True)
        f_new()
        say("#   %s: %s %s" % (what, {k: round(v, 3) for k, v in e.last_timing()[0].items() if v}, e.last_kernels().get("decode")))
        e.set_profiling(False)

    if "shapes" in parts:
        for n_seg, length in ((16, 65536), (64, 16384), (256, 4096), (1024, 1024), (4096, 256), (1, 1 << 20)):
            shape("%d x %d" % (n_seg, length), np.arange(n_seg + 1, dtype=np.int64) * length)
        lens = np.concatenate([rng.integers(200, 2001, size=1000), [1 << 18]])
        lens = lens[rng.permutation(len(lens))]
        padded = 0                                                        # what the classes cost: padded slots over terms, from the plan's notes
        shape("ragged 1000 x 200..2000 + 2^18", np.concatenate([[0], np.cumsum(lens)]))
        for nm in e.last_kernels().get("decode", []):
            if nm.startswith("k_pip_prepare_csr"):
                kv = dict(x.split("=") for x in nm.split("@")[1].split(","))
                padded += int(kv["K"]) * int(kv["n"])
        say("#   ragged: %d terms in runs' slots of %d: padding x %.3f" % (int(lens[lens > 192].sum()), padded, padded / float(lens[lens > 192].sum())))
        shape("16 x 65536 shared points", np.arange(17, dtype=np.int64) * 65536, shared_len=65536)
    if "few" in parts:
        for n_seg in (4, 16):
            for length in (256, 1024, 4096):
                shape("%d x %d" % (n_seg, length), np.arange(n_seg + 1, dtype=np.int64) * length)
    if "pad" in parts:
        say("# what padding costs: the _dev form on resident buffers, every segment padded to max_seg = its length and to twice its length; stream ms")
        for n_seg, length in ((64, 16384), (1024, 1024), (4096, 256)):
            t = n_seg * length
            d_off = torch.from_numpy((np.arange(n_seg + 1, dtype=np.int64) * length).astype(np.int32)).to("cuda:0")
            d_st8 = torch.zeros((n_seg,), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            routes = []
            for factor in (1, 2):
                f = lambda factor=factor: e.msm_optional_many_dev(n_seg, d_off.data_ptr(), d_sc.data_ptr(), None, d_pts.data_ptr(), t, t, factor * length,
                                                                  d_out.data_ptr(), d_st8.data_ptr())
                def s_(f=f):
                    t_ms = profiled(e, f)()
                    e.synchronize()
                    return t_ms
                routes.append(("max_seg = %d x length" % factor, s_, None))
            res = measure(routes)
            for name, _, _ in routes:
                say("%-16s %-22s stream %s ms" % ("%d x %d" % (n_seg, length), name, spread(res[name][0])))
            a, b = (float(np.median(res[r[0]][0])) for r in routes)
            say("%-16s   padded to twice the length: x %.3f (medians), %.3f ms more" % ("%d x %d" % (n_seg, length), b / a, b - a))
    e.close()

    if "cap" in parts:
        eh = Engine(0, test_hooks=True)
        say("# run cap (ZKP_TESTOPT_PIP_RUN_CAP, test-hook build): equal-length jobs of 2^21 terms, point per term; stream ms (the whole call: a call of more than "
            "seven runs keeps moving its last timing mark) and ns per term; call = the synchronous host-pointer call, copies included")
        for n_seg, length in ((32, 65536), (128, 16384), (512, 4096), (2048, 1024)):
            t = n_seg * length
            off = (np.arange(n_seg + 1, dtype=np.int64) * length).astype(np.uint32)
            f = lambda: eh.msm_optional_many(off, sc[:t], pts[:t], None)
            routes = []
            for cap_bits in (21, 20, 19, 18, 17, 16):
                def s(cap_bits=cap_bits):
                    eh.set_option(ZKP_TESTOPT_PIP_RUN_CAP, 1 << cap_bits)
                    return profiled(eh, f)()
                def call_(cap_bits=cap_bits):
                    eh.set_option(ZKP_TESTOPT_PIP_RUN_CAP, 1 << cap_bits)
                    f()
                routes.append(("cap 2^%d: %d runs" % (cap_bits, max(1, t >> cap_bits)), s, call_))
            res = measure(routes)
            for name, _, _ in routes:
                say("%-16s %-22s stream %s ms  (%.2f ns per term, median)  call %s ms" % ("%d x %d" % (n_seg, length), name, spread(res[name][0]),
                                                                                         1e6 * float(np.median(res[name][0])) / t, spread(res[name][1])))
        eh.set_option(ZKP_TESTOPT_PIP_RUN_CAP, 0)
        eh.close()
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()

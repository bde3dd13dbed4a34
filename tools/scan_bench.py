#!/usr/bin/env python3
"""Segmented prefix sums and products of scalars and running sums of points (zkp_mi355x.h (13)) on one MI355X against the routes callers had
before, everything in one process with the routes alternated inside every round.

    python tools/scan_bench.py [scalars] [points] [sweep] [--out FILE]

    scalars  SUM (inclusive) and PRODUCT (exclusive: tables of powers) at one segment of 2^12, 2^16 and 2^20 terms, 64 x 1,024, 4,096 x 32 and
             65,536 x 2: zkp_sc_scan_dev on resident buffers (`stream`: the time between HIP events around what the call queues), the synchronous
             host-pointer zkp_sc_scan (`call`: wall time, copies included), the host backend at 16 threads, and what callers had before: all
             prefixes as one zkp_sc_reduce job (scalar_sum; scalar_product with repeated indices for the powers), which is quadratic in the
             segment length and is measured up to 40 million terms
    points   zkp_scan_points at the same shapes against all prefixes as one zkp_sum_points job (up to 40 million terms), the loop of one
             point_add call per position (up to 4,096 calls) and the host backend at 16 threads
    sweep    what the toolbox defaults are read from: the synchronous device call against the host backend at 16 threads, scalars at 2^12 .. 2^22
             terms and points at 2^6 .. 2^18, in segments of 2, 32, 1,024 terms and one segment

Without a part all three run.  Scalars are random 256-bit values, points random multiples of the basepoint.  Five rounds; min / median / max are
printed, and the spread is the margin of every comparison.  The report goes to stdout and, with --out, to the end of FILE as well."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

OPS = ("SUM", "PRODUCT")
SHAPES = ((1, 1 << 12), (1, 1 << 16), (1, 1 << 20), (64, 1024), (4096, 32), (65536, 2))
QUADRATIC_MAX_TERMS = 40_000_000
LOOP_MAX_CALLS = 4096
ROUNDS = 5
_out = None


def say(line):
    print(line, flush=True)
    if _out is not None:
        _out.write(line + "\n")
        _out.flush()


def spread(v):
    return "%9.3f / %9.3f / %9.3f" % (min(v), float(np.median(v)), max(v))


def wall(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def alternate(routes, rounds=ROUNDS):
    """routes = [(name, timed call returning ms)] -> {name: [ms per round]}, every route once per round in turn, after two warm-up calls each"""
    for _, f in routes:
        f()
        f()
    res = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, f in routes:
            res[name].append(f())
    return res


def verdict(a, b):
    return "ahead beyond the spread" if max(a) < min(b) else ("behind beyond the spread" if min(a) > max(b) else "within the spread")


def prefix_job(n_seg, length, exclusive):
    """(off, idx) of the job that folds every prefix of every segment on its own: row (s, k) references the terms s length + [0, k] (or [0, k))"""
    lens = np.tile(np.arange(length, dtype=np.int64) + (0 if exclusive else 1), n_seg)
    off = np.concatenate([[0], np.cumsum(lens)])
    start = np.repeat(np.arange(n_seg, dtype=np.int64) * length, length)
    idx = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], lens) + np.repeat(start, lens)
    return off.astype(np.uint32), idx.astype(np.uint32)


def main():
    global _out
    import torch
    torch.cuda.init()                                                    # torch's HIP runtime first, as in bench.py
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    args = sys.argv[1:]
    if "--out" in args:
        _out = open(args[args.index("--out") + 1], "a")
        del args[args.index("--out"):args.index("--out") + 2]
    parts = args or ["scalars", "points", "sweep"]
    rng = np.random.default_rng(13)
    eng = Engine(0)
    lib = eng._lib
    say("# one MI355X; parts: %s; %d rounds, routes alternated in one process; min / median / max in ms" % (" ".join(parts), ROUNDS))
    say("# zkp_sc_scan_group() = %d, launches at 2^12, 2^16, 2^20 terms: %d, %d, %d; zkp_scan_points_group() = %d, launches: %d, %d, %d" % (
        lib.zkp_sc_scan_group(), lib.zkp_sc_scan_launches(1 << 12), lib.zkp_sc_scan_launches(1 << 16), lib.zkp_sc_scan_launches(1 << 20),
        lib.zkp_scan_points_group(), lib.zkp_scan_points_launches(1 << 12), lib.zkp_scan_points_launches(1 << 16), lib.zkp_scan_points_launches(1 << 20)))
    n_max = 1 << 22
    A = rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8)
    P = eng.mul_base(A[:1 << 20])
    dA, dP = torch.from_numpy(A).to("cuda:0"), torch.from_numpy(P).to("cuda:0")
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)

    def events(f):
        with torch.cuda.stream(stream):
            ev0.record()
            f()
            ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    def report(what, routes, res, new, olds):
        for rname, _ in routes:
            say("%s %-36s %s" % (what, rname, spread(res[rname])))
        for old in olds:
            if old in res:
                say("%s %s against %s: x %.2f (medians), %s" % (what, new, old, np.median(res[old]) / np.median(res[new]), verdict(res[new], res[old])))

    if "scalars" in parts:
        for op, name in enumerate(OPS):
            excl = op == 1
            for n_seg, length in SHAPES:
                t = n_seg * length
                off = np.arange(0, t + 1, length, dtype=np.uint32)
                a = A[:t]
                d_off = torch.from_numpy(off.view(np.int32)).to("cuda:0")
                d_out = torch.zeros((t, 32), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                routes = [("scan, resident (stream)", lambda: events(lambda: eng.scalar_scan_dev(op, int(excl), n_seg, d_off.data_ptr(), dA.data_ptr(), t, None, t, d_out.data_ptr()))),
                          ("scan, synchronous call", lambda: wall(lambda: eng.scalar_scan(op, off, a, None, excl))),
                          ("scan, host backend, 16 threads", lambda: wall(lambda: T.scalar_scan(None, op, off, a, None, excl, threads=16)))]
                quad = n_seg * length * (length + 1) // 2
                if quad <= QUADRATIC_MAX_TERMS:
                    q_off, q_idx = prefix_job(n_seg, length, excl)
                    dq_off, dq_idx = torch.from_numpy(q_off.view(np.int32)).to("cuda:0"), torch.from_numpy(q_idx.view(np.int32)).to("cuda:0")
                    torch.cuda.synchronize()
                    routes += [("all prefixes as folds, resident", lambda: events(lambda: eng.scalar_reduce_dev(op, t, dq_off.data_ptr(), dA.data_ptr(), t, dq_idx.data_ptr(), None, 0, None,
                                                                                                           int(q_off[-1]), d_out.data_ptr()))),
                               ("all prefixes as folds, synchronous", lambda: wall(lambda: eng.scalar_reduce(op, q_off, a, q_idx)))]
                res = alternate(routes)
                what = "%-8s %6d x %-8d" % (name, n_seg, length)
                report(what, routes[:1], res, "scan, resident (stream)", ["all prefixes as folds, resident"])
                report(what, routes[1:], res, "scan, synchronous call", ["scan, host backend, 16 threads", "all prefixes as folds, synchronous"])
                if quad > QUADRATIC_MAX_TERMS:
                    say("%s all prefixes as folds: %d terms, not measured (above %d)" % (what, quad, QUADRATIC_MAX_TERMS))
                else:
                    assert (eng.scalar_scan(op, off, a, None, excl) == eng.scalar_reduce(op, q_off, a, q_idx)).all()
                if n_seg == 1 and length == 1 << 20:
                    ms = float(np.median(res["scan, resident (stream)"]))
                    say("%s resident stream median %.4f ms for %d bytes read twice and written once: %.1f GB/s" % (what, ms, 32 * t, 96 * t / ms / 1e6))

    if "points" in parts:
        for n_seg, length in SHAPES:
            t = n_seg * length
            off = np.arange(0, t + 1, length, dtype=np.uint32)
            p = P[:t]
            d_off = torch.from_numpy(off.view(np.int32)).to("cuda:0")
            d_out = torch.zeros((t, 32), dtype=torch.uint8, device="cuda:0")
            d_st = torch.zeros(t, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            routes = [("scan, resident (stream)", lambda: events(lambda: eng.point_scan_dev(0, n_seg, d_off.data_ptr(), None, None, dP.data_ptr(), t, t, d_out.data_ptr(), d_st.data_ptr()))),
                      ("scan, synchronous call", lambda: wall(lambda: eng.point_scan(off, p))),
                      ("scan, host backend, 16 threads", lambda: wall(lambda: T.point_cumsum(None, off, p, threads=16)))]
            quad = n_seg * length * (length + 1) // 2
            if quad <= QUADRATIC_MAX_TERMS:
                q_off, q_idx = prefix_job(n_seg, length, False)
                dq_off, dq_idx = torch.from_numpy(q_off.view(np.int32)).to("cuda:0"), torch.from_numpy(q_idx.view(np.int32)).to("cuda:0")
                torch.cuda.synchronize()
                routes += [("all prefixes as sums, resident", lambda: events(lambda: eng.sum_points_dev(t, dq_off.data_ptr(), dq_idx.data_ptr(), None, dP.data_ptr(), t, int(q_off[-1]),
                                                                                                    d_out.data_ptr(), d_st.data_ptr()))),
                           ("all prefixes as sums, synchronous", lambda: wall(lambda: eng.sum_points(q_off, p, q_idx)))]
            if length <= LOOP_MAX_CALLS:
                cols = np.ascontiguousarray(p.reshape(n_seg, length, 32).transpose(1, 0, 2))       # [position][segment]

                def loop():
                    acc = cols[0]
                    for k in range(1, length):
                        acc = eng.add_points(acc, cols[k])[0]
                    return acc
                routes.append(("loop of point_add calls, synchronous", lambda: wall(loop)))
            res = alternate(routes)
            what = "POINTS   %6d x %-8d" % (n_seg, length)
            report(what, routes[:1], res, "scan, resident (stream)", ["all prefixes as sums, resident"])
            report(what, routes[1:], res, "scan, synchronous call", ["scan, host backend, 16 threads", "all prefixes as sums, synchronous", "loop of point_add calls, synchronous"])
            if quad > QUADRATIC_MAX_TERMS:
                say("%s all prefixes as sums: %d terms, not measured (above %d)" % (what, quad, QUADRATIC_MAX_TERMS))
            if length > LOOP_MAX_CALLS:
                say("%s loop of point_add calls: %d calls, not measured (above %d)" % (what, length, LOOP_MAX_CALLS))
            eng.set_profiling(True)
            eng.point_scan(off, p)
            ms, total = eng.last_timing()
            say("%s kernel time by class: decode %.3f, walks %.3f, encode %.3f ms" % (what, ms["decode"], ms["reduce"], ms["combine"]))
            eng.set_profiling(False)

    if "sweep" in parts:
        say("# sweep: synchronous device call against the host backend at 16 threads")
        jobs = [(name, op, range(12, 23, 2)) for op, name in enumerate(OPS)] + [("POINTS", None, range(6, 19, 2))]
        for name, op, bits_range in jobs:
            ahead = {}
            for bits in bits_range:
                t = 1 << bits
                cell = []
                for length in sorted({v for v in (2, 32, 1024, t) if v <= t}):
                    off = np.arange(0, t + 1, length, dtype=np.uint32)
                    if op is None:
                        x = P[:t]
                        routes = [("device", lambda: wall(lambda: eng.point_scan(off, x))), ("host16", lambda: wall(lambda: T.point_cumsum(None, off, x, threads=16)))]
                    else:
                        x = A[:t]
                        routes = [("device", lambda: wall(lambda: eng.scalar_scan(op, off, x, None, op == 1))),
                                  ("host16", lambda: wall(lambda: T.scalar_scan(None, op, off, x, None, op == 1, threads=16)))]
                    res = alternate(routes)
                    v = verdict(res["device"], res["host16"])
                    cell.append(v == "ahead beyond the spread")
                    say("%-8s 2^%-2d terms in segments of %-8d device %s  host16 %s  device %s" % (name, bits, length, spread(res["device"]), spread(res["host16"]), v))
                ahead[bits] = all(cell)
            sizes = sorted(ahead)
            first = next((b for i, b in enumerate(sizes) if all(ahead[c] for c in sizes[i:])), None)
            say("# %s: the synchronous device call is ahead beyond the spread at every mix from %s" % (name, "2^%d terms on" % first if first else "no measured size on: never"))
    eng.close()
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()

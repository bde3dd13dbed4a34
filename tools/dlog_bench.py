#!/usr/bin/env python3
"""Bounded discrete logarithms to the basepoint (zkp_mi355x.h (10)) on one MI355X, against the route callers had before -- basepoint_mul of all
2^bits candidates and a numpy row search -- and against the host backend at 1 and 16 threads on both sides of the toolbox's routing rule, all in
one process.

    python tools/dlog_bench.py [--quick] [--ab LIB ...]

Shapes: 1, 4,096 and 65,536 points at bits 16, 24 and 32, and 4,096 points at bits 40; logarithms uniform in the range, and all small (below 97).
Per shape: `stream` = the time between HIP events around everything the call queues on its stream (zkp_ctx_last_timing's total: every kernel of
the call and the gaps between them, no copies), `call` = the synchronous host-pointer call, copies included.  Each shape is warmed up, then
measured for five rounds (three at 40 bits); min / median / max over the rounds are printed.  A shape whose first call takes
longer than 2 s is measured once (the count is printed).  The old route is run where its table fits (bits <= 24) and said to stop where it does not.
Also: the prepare time and the table bytes per baby_bits, the same shapes at other table sizes (the A/B rows behind the default), and with
--ab LIB the same rows on a library built with another -DZKP_DLOG_CHUNK / -DZKP_DLOG_SLICE_ITEMS (a process of its own per library: this script
starts itself once per LIB)."""
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def spread(v):
    return "%10.3f / %10.3f / %10.3f" % (min(v), float(np.median(v)), max(v))


def time_call(eng, f, reps):
    """(stream ms [k], call ms [k]) of f on eng after one warm call; k = reps, or 1 when the warm call took more than 2 s"""
    t0 = time.perf_counter()
    f()
    if time.perf_counter() - t0 > 2.0:
        reps = 1
    ks, cs = [], []
    for _ in range(reps):
        eng.set_profiling(True)
        f()
        ks.append(eng.last_timing()[1])
        eng.set_profiling(False)
        t0 = time.perf_counter()
        f()
        cs.append(1e3 * (time.perf_counter() - t0))
    return ks, cs


def points_for(eng, ks):
    rows = np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), np.uint8).reshape(-1, 32).copy()
    return eng.mul_base(rows)


def logs(rng, n, bits, small):
    return rng.integers(0, min(97, 1 << bits), size=n) if small else rng.integers(0, 1 << bits, size=n)


def old_route_call(eng, pts, bits):
    """what examples/elgamal_tally_batch.py does, with a sorted search instead of a row-by-row comparison: k B for every k in range, then the rows"""
    sc = np.zeros((1 << bits, 32), np.uint8)
    sc[:, :8] = np.arange(1 << bits, dtype="<u8").view(np.uint8).reshape(-1, 8)
    table = eng.mul_base(sc)
    view = np.ascontiguousarray(table).view("S32").reshape(-1)
    order = np.argsort(view, kind="stable")
    want = np.ascontiguousarray(pts).view("S32").reshape(-1)
    pos = np.searchsorted(view[order], want)
    pos[pos >= len(order)] = 0
    return order[pos]


def shape_rows(eng, rng, shapes, reps, tag=""):
    for n, bits, small in shapes:
        ks = logs(rng, n, bits, small)
        pts = points_for(eng, ks)
        got, st = eng.dlog_base(pts, bits)
        assert not st.any() and (got == ks.astype(np.uint64)).all()
        k, c = time_call(eng, lambda: eng.dlog_base(pts, bits), reps)
        print("%sn = %6d bits = %2d %-8s baby_bits = %2d  stream min/med/max %s ms  call %s ms  (%d rounds)"
              % (tag, n, bits, "small" if small else "uniform", eng.dlog_baby_bits, spread(k), spread(c), len(k)), flush=True)


def ab_main(lib_path, quick):
    from zkp_amd import engine as E
    E.LIB_PATH = lib_path
    eng = E.Engine(0)
    lib = eng._lib
    tag = "A/B chunk = %d slice_chunks(1) = %d: " % (lib.zkp_dlog_chunk(), lib.zkp_dlog_slice_chunks(1))
    rng = np.random.default_rng(7)
    eng.prepare_dlog(16)
    shape_rows(eng, rng, ab_shapes(quick), 5, tag)
    eng.close()


def ab_shapes(quick):
    return [(1, 32, False), (4096, 24, False), (4096, 24, True)] + ([] if quick else [(4096, 32, False), (65536, 24, False)])


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    if "--ab-child" in args:
        ab_main(args[args.index("--ab-child") + 1], quick)
        return
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    eng = Engine(0)
    lib = eng._lib
    rng = np.random.default_rng(7)
    print("# one MI355X; stream = HIP events around the call's stream work; call = synchronous host-pointer call; min / median / max over the rounds")
    print("# zkp_dlog_group() = %d  zkp_dlog_chunk() = %d  zkp_dlog_slice_chunks(1 / 4096 / 65536) = %d / %d / %d"
          % (lib.zkp_dlog_group(), lib.zkp_dlog_chunk(), lib.zkp_dlog_slice_chunks(1), lib.zkp_dlog_slice_chunks(4096), lib.zkp_dlog_slice_chunks(65536)))
    print("# --- prepare: time of zkp_ctx_prepare_dlog (rows on the device, slots on the host) and table bytes")
    for bb in (8, 12, 16, 20) + (() if quick else (22,)):
        ts = []
        for _ in range(3):
            eng.prepare_dlog(4)
            t0 = time.perf_counter()
            eng.prepare_dlog(bb)
            ts.append(1e3 * (time.perf_counter() - t0))
        print("prepare baby_bits = %2d  min/med/max %s ms  rows %d B + slots %d B" % (bb, spread(ts), 32 << bb, 16 << bb), flush=True)
    print("# --- the default table (a fresh context's first call builds it)")
    fresh = Engine(0)
    fresh.dlog_base(points_for(eng, [5]), 8)
    default = fresh.dlog_baby_bits
    fresh.close()
    print("default baby_bits =", default)
    eng.prepare_dlog(default)
    shapes = [(n, bits, small) for bits in (16, 24, 32) for n in (1, 4096, 65536) for small in (False, True)]
    if quick:
        shapes = [s for s in shapes if not (s[0] == 65536 and s[1] == 32 and not s[2])]
    shape_rows(eng, rng, shapes, 5)
    print("# --- bits = 40")
    eng.prepare_dlog(22 if not quick else 20)
    shape_rows(eng, rng, [(1, 40, False), (4096, 40, True)] + ([] if quick else [(4096, 40, False)]), 3)
    print("# --- other table sizes on the same shapes (the A/B rows behind the default)")
    for bb in (12, 20):
        eng.prepare_dlog(bb)
        shape_rows(eng, rng, [(1, 24, False), (4096, 24, False), (4096, 24, True), (65536, 16, False), (1, 32, False)] + ([] if bb == 12 else [(4096, 32, False)]), 5)
    eng.prepare_dlog(default)
    eng.set_profiling(True)
    ks = logs(rng, 4096, 24, False)
    eng.dlog_base(points_for(eng, ks), 24)
    print("# kernels of n = 4096 bits = 24:", eng.last_kernels(), {k: round(v, 3) for k, v in eng.last_timing()[0].items() if v})
    eng.set_profiling(False)
    print("# --- the route callers had: basepoint_mul of all 2^bits candidates + a sorted row search in numpy (4,096 points)")
    for bits in (16, 20) + (() if quick else (24,)):
        ks = logs(rng, 4096, bits, False)
        pts = points_for(eng, ks)
        assert (old_route_call(eng, pts, bits) == ks).all()
        ts = []
        for _ in range(3 if bits < 24 else 1):
            t0 = time.perf_counter()
            old_route_call(eng, pts, bits)
            ts.append(1e3 * (time.perf_counter() - t0))
        k, c = time_call(eng, lambda: eng.dlog_base(pts, bits), 5)
        print("old route n = 4096 bits = %2d  call min/med/max %s ms (table of %d MB)  against dlog_base call %s ms" % (bits, spread(ts), (32 << bits) >> 20, spread(c)), flush=True)
    print("# bits = 28 and beyond: the old route needs 32 B x 2^bits of host memory for the table (8 GB at 28, 128 GB at 32) and was not run")
    bb, per_thread = T.get_dlog_baby_bits(), T.get_dlog_host_max_steps()
    print("# --- the host backend at 1 and 16 threads (table of 2^%d rows) against the device call, on both sides of the routing rule: a call stays on the" % bb)
    print("#     host while its work n (2^(bits - %d) + 128) is at most %d giant steps per thread (threads counted up to 16)" % (bb, per_thread))
    host_shapes = {1: ((1, 16), (7, 16), (14, 16), (15, 16), (16, 16), (1, 22), (1, 23), (1, 24)),
                   16: ((1, 16), (16, 16), (113, 16), (227, 16), (228, 16), (256, 16), (1, 24), (1, 26), (1, 27), (4096, 16), (4096, 24)) + (() if quick else ((1, 32),))}
    for threads in (1, 16):
        for n, bits in host_shapes[threads]:
            ks = logs(rng, n, bits, False)
            pts = points_for(eng, ks)
            T.basepoint_dlog(None, pts, bits, threads=threads)
            ts = []
            for _ in range(5 if n * (1 << max(0, bits - bb)) < (1 << 22) else 3):
                t0 = time.perf_counter()
                T.basepoint_dlog(None, pts, bits, threads=threads)
                ts.append(1e3 * (time.perf_counter() - t0))
            k, c = time_call(eng, lambda: eng.dlog_base(pts, bits), 5)
            work = n * ((1 << max(0, bits - bb)) + 128)
            print("host threads = %2d n = %5d bits = %2d work = %9d (%s by default)  min/med/max %s ms  against dlog_base call %s ms"
                  % (threads, n, bits, work, "host" if work <= per_thread * min(threads, 16) else "device", spread(ts), spread(c)), flush=True)
    eng.close()
    for path in [args[i + 1] for i, a in enumerate(args) if a == "--ab"]:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", path] + (["--quick"] if quick else []), check=True, timeout=600)


if __name__ == "__main__":
    main()

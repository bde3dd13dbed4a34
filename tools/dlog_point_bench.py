#!/usr/bin/env python3
"""Bounded discrete logarithms to a base of the caller's and over signed ranges (zkp_mi355x.h (10): zkp_dlog_point) on one MI355X, all in one
process, the routes of a row alternated round by round.

    python tools/dlog_point_bench.py [--quick] [--parent LIB]

(a) zkp_dlog_base at the shapes of profiles/dlog_bench.txt -- 1 / 4,096 / 65,536 points at 16, 24, 32 bits, logarithms uniform in range -- on this
    build and, with --parent LIB, on a libzkp_mi355x.so built from the parent commit: both libraries are loaded side by side through the same few
    ctypes calls and take turns within every round.  The kernels this build edited must not have slowed the existing call.
(b) zkp_dlog_point on a slot of B and on a slot of a hashed H at the same shapes, in the same rounds as (a).
(c) signed against unsigned at 32 bits for 4,096 points to base H: logarithms uniform in range; magnitudes below 100 of both signs; and the same
    small magnitudes through the route callers had -- point_add of 2^31 H, then the unsigned call.
(d) the route callers had for another base: point_cumsum of H repeated 2^bits times and a sorted row search, at 16 and 20 bits (4,096 points).
(e) prepare times of a slot at 2^12, 2^16 and 2^20 rows.
Per row: `stream` = the time between HIP events around everything the call queues on its stream (zkp_ctx_last_timing's total), `call` = the
synchronous host-pointer call, copies included; one warm call, then five rounds; min / median / max are printed.  --quick leaves out the shape of
65,536 points at 32 bits uniform (2 s a call)."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROUNDS = 5


def spread(v):
    return "%9.3f / %9.3f / %9.3f" % (min(v), float(np.median(v)), max(v))


class Raw:
    """the few calls (a) needs, bound by hand so that a library of the parent commit loads too"""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        lib.zkp_ctx_create.argtypes, lib.zkp_ctx_create.restype = [ctypes.POINTER(vp), ctypes.c_int], ctypes.c_int
        lib.zkp_ctx_destroy.argtypes, lib.zkp_ctx_destroy.restype = [vp], None
        lib.zkp_ctx_prepare_dlog.argtypes, lib.zkp_ctx_prepare_dlog.restype = [vp, u32], ctypes.c_int
        lib.zkp_dlog_base.argtypes, lib.zkp_dlog_base.restype = [vp, u64, vp, u32, vp, vp], ctypes.c_int
        lib.zkp_ctx_set_profiling.argtypes, lib.zkp_ctx_set_profiling.restype = [vp, ctypes.c_int], ctypes.c_int
        lib.zkp_ctx_last_timing.argtypes, lib.zkp_ctx_last_timing.restype = [vp, vp, vp], ctypes.c_int
        self.h = vp()
        assert lib.zkp_ctx_create(ctypes.byref(self.h), 0) == 0
        assert lib.zkp_ctx_prepare_dlog(self.h, 16) == 0

    def dlog_base(self, pts, bits):
        n = len(pts)
        out, st = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        assert self.lib.zkp_dlog_base(self.h, n, pts.ctypes.data, bits, out.ctypes.data, st.ctypes.data) == 0
        return out, st

    def set_profiling(self, on):
        assert self.lib.zkp_ctx_set_profiling(self.h, int(on)) == 0

    def last_total(self):
        arr, tot = (ctypes.c_float * 32)(), ctypes.c_float()
        assert self.lib.zkp_ctx_last_timing(self.h, arr, ctypes.byref(tot)) >= 0
        return float(tot.value)

    def close(self):
        self.lib.zkp_ctx_destroy(self.h)


class EngRoute:
    """an Engine behind the same three calls"""

    def __init__(self, eng):
        self.eng = eng

    def set_profiling(self, on):
        self.eng.set_profiling(on)

    def last_total(self):
        return self.eng.last_timing()[1]


def alternate(routes, rounds=ROUNDS):
    """routes: [(label, timer object, f)].  One warm call each, then `rounds` rounds in which the routes take turns: {label: (stream ms, call ms)}.
    A route whose warm call takes more than 2 s is measured once."""
    res = {label: ([], []) for label, _, _ in routes}
    slow = False
    for _, _, f in routes:
        t0 = time.perf_counter()
        f()
        slow = slow or time.perf_counter() - t0 > 2.0
    for _ in range(1 if slow else rounds):
        for label, obj, f in routes:
            obj.set_profiling(True)
            f()
            res[label][0].append(obj.last_total())
            obj.set_profiling(False)
            t0 = time.perf_counter()
            f()
            res[label][1].append(1e3 * (time.perf_counter() - t0))
    return res


def show(head, res):
    for label, (k, c) in res.items():
        print("%s %-34s stream min/med/max %s ms  call %s ms  (%d rounds)" % (head, label, spread(k), spread(c), len(k)), flush=True)


def scalar_rows(ks, L):
    return np.frombuffer(b"".join((int(k) % L).to_bytes(32, "little") for k in ks), np.uint8).reshape(-1, 32).copy()


def main():
    args = sys.argv[1:]
    quick = "--quick" in args
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    from zkp_amd import engine as E
    from zkp_amd import toolbox as T
    L = 2**252 + 27742317777372353535851937790883648493
    eng = E.Engine(0)
    er = EngRoute(eng)
    rng = np.random.default_rng(7)
    B = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
    H = T.hash_from_bytes_sha512(None, [b"dlog_point_bench H"])[0]
    print("# one MI355X; stream = HIP events around the call's stream work; call = synchronous host-pointer call; min / median / max over %d rounds;" % ROUNDS)
    print("# the routes of a shape take turns within every round, all in one process.  Tables of 2^16 rows.")
    print("# zkp_dlog_slice_chunks(1 / 4096 / 65536) = %d / %d / %d, signed %d / %d / %d" % tuple(
        [eng._lib.zkp_dlog_slice_chunks(n) for n in (1, 4096, 65536)] + [eng._lib.zkp_dlog_slice_chunks_signed(n) for n in (1, 4096, 65536)]))

    def mul(base, ks):
        out, st = T.point_mul(eng, scalar_rows(ks, L), np.frombuffer(base, np.uint8).reshape(1, 32), 0)
        assert not st.any()
        return out

    print("# --- (e) prepare: time of zkp_ctx_prepare_dlog_point (the base's fixed-base table, rows on the device, slots on the host), base H")
    for bb in (12, 16, 20):
        ts = []
        for _ in range(3):
            eng.release_dlog_point(2)
            t0 = time.perf_counter()
            eng.prepare_dlog_point(2, H, bb)
            ts.append(1e3 * (time.perf_counter() - t0))
        print("(e) prepare slot baby_bits = %2d  min/med/max %s ms" % (bb, spread(ts)), flush=True)
    eng.release_dlog_point(2)

    eng.prepare_dlog(16)
    eng.prepare_dlog_point(0, B, 16)
    eng.prepare_dlog_point(1, H, 16)
    this = Raw(E.LIB_PATH)
    old = Raw(parent) if parent else None
    print("# --- (a) zkp_dlog_base, this build%s; (b) zkp_dlog_point on a slot of B and on a slot of H; logarithms uniform in [0, 2^bits)" % (" against the parent commit's" if old else ""))
    for bits in (16, 24, 32):
        for n in (1, 4096, 65536):
            if quick and n == 65536 and bits == 32:
                continue
            ks = rng.integers(0, 1 << bits, size=n)
            pB, pH = mul(B, ks), mul(H, ks)
            want = ks.astype(np.uint64)
            for got, st in (this.dlog_base(pB, bits), eng.dlog_point(0, pB, bits), eng.dlog_point(1, pH, bits)) + ((old.dlog_base(pB, bits),) if old else ()):
                assert not st.any() and (got == want).all()
            routes = ([("(a) zkp_dlog_base parent", old, lambda: old.dlog_base(pB, bits))] if old else []) + [
                ("(a) zkp_dlog_base this build", this, lambda: this.dlog_base(pB, bits)),
                ("(b) zkp_dlog_point slot of B", er, lambda: eng.dlog_point(0, pB, bits)),
                ("(b) zkp_dlog_point slot of H", er, lambda: eng.dlog_point(1, pH, bits))]
            show("n = %6d bits = %2d" % (n, bits), alternate(routes))
    this.close()
    if old:
        old.close()

    print("# --- (c) signed against unsigned, 4,096 points at 32 bits, base H")
    n, bits = 4096, 32
    half = 1 << (bits - 1)
    ku = rng.integers(0, 1 << bits, size=n)
    ks = rng.integers(-half, half, size=n)
    ksmall = rng.integers(-99, 100, size=n)
    pu, ps, psmall, psmall_pos = mul(H, ku), mul(H, ks), mul(H, ksmall), mul(H, np.abs(ksmall))
    offset = mul(H, [half])

    def workaround():
        shifted, bad = T.point_add(eng, psmall, offset)
        k, st = eng.dlog_point(1, shifted, bits)
        return k.astype(np.int64) - half, st

    for (got, st), want in ((eng.dlog_point(1, ps, bits, signed=True), ks), (eng.dlog_point(1, psmall, bits, signed=True), ksmall), (workaround(), ksmall)):
        assert not st.any() and (got == want).all()
    show("n = %6d bits = %2d" % (n, bits), alternate([
        ("(c) unsigned, uniform", er, lambda: eng.dlog_point(1, pu, bits)),
        ("(c) signed, uniform", er, lambda: eng.dlog_point(1, ps, bits, signed=True)),
        ("(c) unsigned, 0 <= k < 100", er, lambda: eng.dlog_point(1, psmall_pos, bits)),
        ("(c) signed, |k| < 100", er, lambda: eng.dlog_point(1, psmall, bits, signed=True))]))
    # the workaround is two calls: its stream time is the unsigned call's alone, its call time covers both
    show("n = %6d bits = %2d" % (n, bits), alternate([("(c) |k| < 100: point_add 2^31 H + unsigned", er, workaround)]))

    print("# --- (d) the route callers had for another base: point_cumsum of H repeated 2^bits times + a sorted row search in numpy (4,096 points)")

    def old_route(pts, bits):
        cnt = (1 << bits) - 1
        table, bad = T.point_cumsum(eng, [0, cnt], np.frombuffer(H, np.uint8).reshape(1, 32), pidx=np.zeros(cnt, np.uint32))      # row i = (i + 1) H
        view = np.ascontiguousarray(table).view("S32").reshape(-1)
        order = np.argsort(view, kind="stable")
        want = np.ascontiguousarray(pts).view("S32").reshape(-1)
        pos = np.searchsorted(view[order], want)
        pos[pos >= len(order)] = 0
        return order[pos] + 1

    for bits in (16, 20):
        ks = rng.integers(1, 1 << bits, size=4096)
        pts = mul(H, ks)
        assert (old_route(pts, bits) == ks).all()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            old_route(pts, bits)
            ts.append(1e3 * (time.perf_counter() - t0))
        res = alternate([("zkp_dlog_point", er, lambda: eng.dlog_point(1, pts, bits))])
        print("(d) old route n = 4096 bits = %2d  call min/med/max %s ms (table of %d MB)  against zkp_dlog_point call %s ms"
              % (bits, spread(ts), (32 << bits) >> 20, spread(res["zkp_dlog_point"][1])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

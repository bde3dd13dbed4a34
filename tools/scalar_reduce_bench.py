#!/usr/bin/env python3
"""Segmented scalar sums, products and dot products (zkp_mi355x.h (12)) on one MI355X against the routes callers had before, everything in one
process with the routes alternated inside every round.

    python tools/scalar_reduce_bench.py [shapes] [sweep] [matvec] [--out FILE]

    shapes   per op: 65,536 segments of 2 terms, 4,096 of 32, 64 of 1,024, one of 65,536, one of 2^20 -- zkp_sc_reduce_dev on resident buffers
             (`stream`: the time between HIP events around what the call queues), the synchronous host-pointer zkp_sc_reduce (`call`: wall time,
             copies included), the host backend at 16 threads and Python integers on the decoded rows (wall time); and the bytes per second of the
             one-segment SUM of 2^20 terms on resident buffers
    sweep    what the defaults of zkp_toolbox_get_scalar_reduce_min_terms(op) are read from: 2^12 .. 2^22 terms in segments of 2, 32, 1,024 terms and
             one segment, the synchronous device call against the host backend at 16 threads
    matvec   DOT as a matrix-vector job, the Pedersen check acc_i = sum_k w_k m_ki: K = 1,024 weights gathered through aidx against 1,025 columns,
             against the loop of K scalar_muladd calls (synchronous) and of K zkp_sc_muladd_dev calls on resident buffers (stream)

Without a part all three run.  Operands are random 256-bit values.  Five rounds; min / median / max are printed, and the spread is the margin of
every comparison.  The report goes to stdout and, with --out, to the end of FILE as well."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
OPS = ("SUM", "PRODUCT", "DOT")
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


def python_ints(op, off, a, b):
    va = [int.from_bytes(bytes(r), "little") for r in a]
    vb = None if b is None else [int.from_bytes(bytes(r), "little") for r in b]

    def f():
        out = []
        for i in range(len(off) - 1):
            lo, hi = int(off[i]), int(off[i + 1])
            if op == 0:
                out.append(sum(va[lo:hi]) % L)
            elif op == 1:
                acc = 1
                for x in va[lo:hi]:
                    acc = acc * x % L
                out.append(acc)
            else:
                out.append(sum(x * y for x, y in zip(va[lo:hi], vb[lo:hi])) % L)
        return out
    return f


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
    parts = args or ["shapes", "sweep", "matvec"]
    rng = np.random.default_rng(12)
    eng = Engine(0)
    G = eng._lib.zkp_sc_reduce_group()
    say("# one MI355X; parts: %s; %d rounds, routes alternated in one process; min / median / max in ms" % (" ".join(parts), ROUNDS))
    say("# zkp_sc_reduce_group() = %d; levels at 2^16, 2^20, 2^22 terms: %d, %d, %d" % (G, eng._lib.zkp_sc_reduce_levels(1 << 16), eng._lib.zkp_sc_reduce_levels(1 << 20),
                                                                                   eng._lib.zkp_sc_reduce_levels(1 << 22)))
    n_max = 1 << 22
    A = rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8)
    B = rng.integers(0, 256, size=(n_max, 32), dtype=np.uint8)
    dA, dB = torch.from_numpy(A).to("cuda:0"), torch.from_numpy(B).to("cuda:0")
    torch.cuda.synchronize()

    def dev_call(op, off, t):
        n_out = len(off) - 1
        d_off = torch.from_numpy(off.view(np.int32)).to("cuda:0")
        d_out = torch.zeros((n_out, 32), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dot = op == 2

        def f():
            eng.set_profiling(True)
            eng.scalar_reduce_dev(op, n_out, d_off.data_ptr(), dA.data_ptr(), t, None, dB.data_ptr() if dot else None, t if dot else 0, None, t, d_out.data_ptr())
            eng.synchronize()
            ms = eng.last_timing()[1]
            eng.set_profiling(False)
            return ms
        f.keep = (d_off, d_out)
        return f

    if "shapes" in parts:
        for op, name in enumerate(OPS):
            for n_out, length in ((65536, 2), (4096, 32), (64, 1024), (1, 65536), (1, 1 << 20)):
                t = n_out * length
                off = np.arange(0, t + 1, length, dtype=np.uint32)
                a, b = A[:t], (B[:t] if op == 2 else None)
                ints = python_ints(op, off, a, b)
                routes = [("device, resident (stream)", dev_call(op, off, t)),
                          ("device, synchronous call", lambda: wall(lambda: eng.scalar_reduce(op, off, a, None, b))),
                          ("host backend, 16 threads", lambda: wall(lambda: T.scalar_reduce(None, op, off, a, None, b, threads=16))),
                          ("Python integers", lambda: wall(ints))]
                res = alternate(routes)
                what = "%-8s %6d x %-8d" % (name, n_out, length)
                for rname, _ in routes:
                    say("%s %-28s %s" % (what, rname, spread(res[rname])))
                say("%s synchronous call against host backend: x %.2f (medians), %s; against Python integers: x %.2f" % (
                    what, np.median(res["host backend, 16 threads"]) / np.median(res["device, synchronous call"]),
                    verdict(res["device, synchronous call"], res["host backend, 16 threads"]), np.median(res["Python integers"]) / np.median(res["device, synchronous call"])))
                if op == 0 and n_out == 1 and length == 1 << 20:
                    ms = float(np.median(res["device, resident (stream)"]))
                    say("%s resident stream median %.4f ms for %d bytes of terms: %.1f GB/s" % (what, ms, 32 * t, 32 * t / ms / 1e6))
                eng.set_profiling(True)
                eng.scalar_reduce(op, off, a, None, b)
                say("#   kernels: %s" % eng.last_kernels()["scalars"])
                eng.set_profiling(False)

    if "sweep" in parts:
        say("# sweep: synchronous device call against the host backend at 16 threads")
        ahead = {op: {} for op in range(3)}
        for op, name in enumerate(OPS):
            for bits in (12, 14, 16, 18, 20, 22):
                t = 1 << bits
                a, b = A[:t], (B[:t] if op == 2 else None)
                cell = []
                for length in (2, 32, 1024, t):
                    off = np.arange(0, t + 1, length, dtype=np.uint32)
                    routes = [("device", lambda: wall(lambda: eng.scalar_reduce(op, off, a, None, b))),
                              ("host16", lambda: wall(lambda: T.scalar_reduce(None, op, off, a, None, b, threads=16)))]
                    res = alternate(routes)
                    v = verdict(res["device"], res["host16"])
                    cell.append(v == "ahead beyond the spread")
                    say("%-8s 2^%-2d terms in segments of %-8d device %s  host16 %s  device %s" % (name, bits, length, spread(res["device"]), spread(res["host16"]), v))
                ahead[op][bits] = all(cell)
        for op, name in enumerate(OPS):
            sizes = sorted(ahead[op])
            first = next((b for i, b in enumerate(sizes) if all(ahead[op][c] for c in sizes[i:])), None)
            say("# %s: the synchronous device call is ahead beyond the spread at every mix from %s" % (name, "2^%d terms on" % first if first else "no measured size on: never"))

    if "matvec" in parts:
        K, cols = 1024, 1025
        t = K * cols
        w, m = A[:K], B[:t]                                              # m[i K + k] = m_ki: column i contiguous
        off = np.arange(0, t + 1, K, dtype=np.uint32)
        aidx = np.tile(np.arange(K, dtype=np.uint32), cols)
        mk = np.ascontiguousarray(m.reshape(cols, K, 32).transpose(1, 0, 2))           # row-major [k][i] for the loop of muladd calls
        d_w, d_mk = torch.from_numpy(w).to("cuda:0"), torch.from_numpy(mk).to("cuda:0")
        d_acc = torch.zeros((cols, 32), dtype=torch.uint8, device="cuda:0")
        d_off, d_ai = torch.from_numpy(off.view(np.int32)).to("cuda:0"), torch.from_numpy(aidx.view(np.int32)).to("cuda:0")
        d_out = torch.zeros((cols, 32), dtype=torch.uint8, device="cuda:0")
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

        def loop_dev():
            d_acc.zero_()
            for k in range(K):
                eng.scalar_muladd_dev(cols, d_w.data_ptr() + 32 * k, 0, d_mk.data_ptr() + 32 * cols * k, 1, d_acc.data_ptr(), 1, d_acc.data_ptr())

        def loop_sync():
            acc = np.zeros((cols, 32), np.uint8)
            for k in range(K):
                acc = T.scalar_muladd(eng, w[k], mk[k], acc)
            return acc

        def loop_host():
            acc = np.zeros((cols, 32), np.uint8)
            for k in range(K):
                acc = T.scalar_muladd(None, w[k], mk[k], acc)
            return acc

        old = T.get_host_max_terms()
        T.set_host_max_terms(0)
        routes = [("zkp_sc_reduce_dev, resident (stream)", lambda: events(lambda: eng.scalar_reduce_dev(2, cols, d_off.data_ptr(), d_w.data_ptr(), K, d_ai.data_ptr(), dB.data_ptr(), t, None, t, d_out.data_ptr()))),
                  ("loop of K zkp_sc_muladd_dev (stream)", lambda: events(loop_dev)),
                  ("zkp_sc_reduce, synchronous call", lambda: wall(lambda: eng.scalar_reduce(2, off, w, aidx, m))),
                  ("loop of K scalar_muladd, engine", lambda: wall(loop_sync)),
                  ("loop of K scalar_muladd, host", lambda: wall(loop_host)),
                  ("host backend scalar_dot, 16 threads", lambda: wall(lambda: T.scalar_reduce(None, 2, off, w, aidx, m, threads=16)))]
        res = alternate(routes)
        T.set_host_max_terms(old)
        want = T.scalar_reduce(None, 2, off, w, aidx, m, threads=16)
        assert (d_out.cpu().numpy() == want).all() and (d_acc.cpu().numpy() == want).all() and (loop_sync() == want).all()
        for rname, _ in routes:
            say("DOT matvec K = %d x %d columns   %-40s %s" % (K, cols, rname, spread(res[rname])))
        say("DOT matvec: resident, one call against the loop: x %.1f (medians), %s; synchronous, one call against the loop on the engine: x %.1f, %s" % (
            np.median(res["loop of K zkp_sc_muladd_dev (stream)"]) / np.median(res["zkp_sc_reduce_dev, resident (stream)"]),
            verdict(res["zkp_sc_reduce_dev, resident (stream)"], res["loop of K zkp_sc_muladd_dev (stream)"]),
            np.median(res["loop of K scalar_muladd, engine"]) / np.median(res["zkp_sc_reduce, synchronous call"]),
            verdict(res["zkp_sc_reduce, synchronous call"], res["loop of K scalar_muladd, engine"])))
        say("DOT matvec: synchronous call against the host backend's scalar_dot at 16 threads: x %.2f, %s" % (
            np.median(res["host backend scalar_dot, 16 threads"]) / np.median(res["zkp_sc_reduce, synchronous call"]),
            verdict(res["zkp_sc_reduce, synchronous call"], res["host backend scalar_dot, 16 threads"])))
    eng.close()
    if _out is not None:
        _out.close()


if __name__ == "__main__":
    main()

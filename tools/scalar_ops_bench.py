#!/usr/bin/env python3
"""Batched scalars mod l (zkp_mi355x.h (6)) on one MI355X: Scalar::invert, from_bytes_mod_order_wide, a * b + c and
Scalar::hash_from_bytes::<Sha512> for batches of 4,096, 65,536 and 2^20.

    python tools/scalar_ops_bench.py        # per operation and size: kernel time from HIP events (zkp_ctx_last_timing; kind scalars, the hash
                                            # under kind transcript), median of 20 calls; the synchronous host-pointer call; the host backend
                                            # at 16 threads; for inversion the route callers had before (pow(x, -1, L) per element in
                                            # Python) at 65,536; the smallest n of 16 .. 4,096 at which the device call beats the host backend
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SIZES = (4096, 65536, 1 << 20)
CROSS = (16, 64, 256, 1024, 4096)
REPS = 20
L = 2**252 + 27742317777372353535851937790883648493


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def operations(eng, T, n, rng):
    """name -> (device call, host-backend call at 16 threads, timing kind)"""
    A, B, Cc = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(3))
    W = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    ops = {"invert": (lambda: eng.scalar_invert(A), lambda: T.scalar_invert(None, A, threads=16), "scalars"),
           "from_wide": (lambda: eng.scalar_from_wide(W), lambda: T.scalar_from_wide(None, W, threads=16), "scalars"),
           "muladd": (lambda: eng.scalar_muladd(A, B, Cc), lambda: T.scalar_muladd(None, A, B, Cc, threads=16), "scalars")}
    for length in (32, 1024):
        data = rng.integers(0, 256, size=n * length, dtype=np.uint8)
        offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
        ops["hash %4d B" % length] = (lambda d=data, o=offsets: eng.scalar_hash_from_bytes_sha512_csr(d, o),
                                      lambda d=data, o=offsets: T.scalar_hash_from_bytes_sha512_csr(None, d, o, threads=16), "transcript")
    return ops, A


def main():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    rng = np.random.default_rng(252)
    eng = Engine(0)
    print("# one MI355X; kernel = HIP events (zkp_ctx_last_timing), median of %d calls; call = the synchronous host-pointer call, copies "
          "included, median of %d; host = the host backend at 16 threads, median of 3" % (REPS, REPS))
    for n in SIZES:
        ops, A = operations(eng, T, n, rng)
        for name, (dev, host, kind) in ops.items():
            dev()                                                       # warm: workspace, code objects
            eng.set_profiling(True)
            k = []
            for _ in range(REPS):
                dev()
                k.append(eng.last_timing()[0][kind])
            eng.set_profiling(False)
            km = float(np.median(k))
            call = median_ms(dev, REPS)
            th = median_ms(host, 3)
            print("%-11s n = %8d   kernel %9.3f ms = %8.2f M outputs/s   call %9.3f ms   host backend 16 threads %9.2f ms = %7.3f M outputs/s"
                  % (name, n, km, n / km / 1e3, call, th, n / th / 1e3))
        if n == 65536:
            vals = [int.from_bytes(bytes(r), "little") % L or 1 for r in A]
            t0 = time.perf_counter()
            out = b"".join(pow(v, -1, L).to_bytes(32, "little") for v in vals)
            print("invert      n = %8d   pow(x, -1, L) per element in Python %9.1f ms = %7.3f M outputs/s" % (n, 1e3 * (time.perf_counter() - t0), n / (1e3 * (time.perf_counter() - t0)) / 1e3))
            del out
    print("# crossover: the synchronous device call against the host backend at 16 threads (median of 20 each), n = " + ", ".join(map(str, CROSS)))
    first = {}
    for n in CROSS:
        ops, _ = operations(eng, T, n, rng)
        for name, (dev, host, _) in ops.items():
            dev()
            host()
            td, th = median_ms(dev, REPS), median_ms(host, REPS)
            if td < th:
                first.setdefault(name, n)
            print("%-11s n = %5d   device call %8.3f ms   host backend %8.3f ms" % (name, n, td, th))
    for name in ops:
        print("# %-11s the device call beats the host backend from n = %s (shared host_max_terms default: %d)"
              % (name, first.get(name, "above 4096"), T.get_host_max_terms()))
    eng.close()


if __name__ == "__main__":
    main()

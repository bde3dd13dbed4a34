#!/usr/bin/env python3
"""RistrettoPoint::hash_from_bytes::<Sha512> for a batch (zkp_mi355x.h (5), zkp_hash_from_bytes_sha512) on one MI355X: what SHA-512
(k_sha512_csr) adds to the map (k_from_uniform), and what the batched call saves over hashing in Python.

    python tools/hash_from_bytes_bench.py            # per size: kernel times from HIP events (SHA-512 stage = kind transcript, map = kind
                                                     # decode), median of 20 calls; from_uniform_bytes alone at the same n; the host
                                                     # backend at 16 threads; the old route (hashlib per message in Python, then the map)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/hash_from_bytes_bench.py --trace
                                                     # the same calls, a few of each, for the kernel trace (a run of its own)

Sizes: 2^20 messages of 32 bytes, 65,536 of 1 KiB, and 4,096 of 32 bytes (a lone call)."""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SIZES = ((1 << 20, 32), (65536, 1024), (4096, 32))
REPS = 20


def batch(n, length, rng):
    data = rng.integers(0, 256, size=n * length, dtype=np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
    return data, offsets


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def bench():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    rng = np.random.default_rng(512)
    eng = Engine(0)
    print("# one MI355X; kernel times from HIP events (zkp_ctx_last_timing), median of %d calls; call = the synchronous host-pointer call, "
          "copies included" % REPS)
    for n, length in SIZES:
        data, offsets = batch(n, length, rng)
        wide = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        eng.hash_from_bytes_sha512_csr(data, offsets)                   # warm: workspace, code objects
        eng.from_uniform_bytes(wide)
        eng.set_profiling(True)
        sha, mp, tot, fub = [], [], [], []
        for _ in range(REPS):
            eng.hash_from_bytes_sha512_csr(data, offsets)
            t = eng.last_timing()[0]
            sha.append(t["transcript"])
            mp.append(t["decode"])
            tot.append(t["transcript"] + t["decode"])
            eng.from_uniform_bytes(wide)
            fub.append(eng.last_timing()[0]["decode"])
        eng.set_profiling(False)
        call = median_ms(lambda: eng.hash_from_bytes_sha512_csr(data, offsets), REPS)
        k, s, m, f = (float(np.median(x)) for x in (tot, sha, mp, fub))
        print("n = %8d x %4d B   hash_from_bytes kernels %8.3f ms = %7.2f M outputs/s (sha512 %7.3f ms, map %7.3f ms)   "
              "from_uniform_bytes alone %8.3f ms = %7.2f M outputs/s   ratio %.3f   call %8.3f ms"
              % (n, length, k, n / k / 1e3, s, m, f, n / f / 1e3, k / f, call))
    for n, length in ((65536, 32), (4096, 1024)):
        data, offsets = batch(n, length, rng)
        msgs = [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]
        t_host = median_ms(lambda: T.hash_from_bytes_sha512_csr(None, data, offsets, threads=16), 3)
        old_hash = median_ms(lambda: b"".join(hashlib.sha512(m).digest() for m in msgs), 3)
        wide = np.frombuffer(b"".join(hashlib.sha512(m).digest() for m in msgs), np.uint8).reshape(-1, 64)
        old_map = median_ms(lambda: eng.from_uniform_bytes(wide), 3)
        t_dev = median_ms(lambda: eng.hash_from_bytes_sha512_csr(data, offsets), 3)
        print("n = %8d x %4d B   host backend 16 threads %8.1f ms = %6.3f M outputs/s   old route (hashlib in Python %7.1f ms + device map "
              "%6.1f ms) %8.1f ms = %6.3f M outputs/s   device call %7.1f ms"
              % (n, length, t_host, n / t_host / 1e3, old_hash, old_map, old_hash + old_map, n / (old_hash + old_map) / 1e3, t_dev))
    eng.close()


def trace():
    from zkp_amd.engine import Engine
    rng = np.random.default_rng(512)
    eng = Engine(0)
    for n, length in SIZES:
        data, offsets = batch(n, length, rng)
        wide = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        for _ in range(5):
            eng.hash_from_bytes_sha512_csr(data, offsets)
            eng.from_uniform_bytes(wide)
        print("traced n = %d x %d B: 5 x (k_sha512_csr + k_from_uniform), 5 x k_from_uniform alone" % (n, length))
    eng.close()


if __name__ == "__main__":
    trace() if "--trace" in sys.argv else bench()

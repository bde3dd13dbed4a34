#!/usr/bin/env python3
"""Batched Merlin operations (zkp_mi355x.h (7)) on one MI355X: append_message for 4,096 and 65,536 transcripts with messages of 32 bytes,
of 0..599 bytes (the mix of profiles/ragged_transcripts_bench.txt) and of 4,096 bytes, and challenge_bytes of 64 bytes.

    python tools/transcript_ops_bench.py [--out FILE]    # per case: kernel time from HIP events (zkp_ctx_last_timing, kind transcript), median
                                            # of 20 calls; the synchronous host-pointer call (copies included) and the route callers had
                                            # before, zkp_transcripts_append_message_batch at 16 threads, measured in the same process and
                                            # alternated, median of 20 each; then the device call against the host threads for 32-byte
                                            # messages from N = 16 up; `routed` = the route the toolbox's default routing takes
                                            # (zkp_ctx_last_kernels).  Every transcript starts from one shared blob
                                            # (Transcript::new(label) per proof, shared_initial = 1); the 0..599-byte mix also runs in place.
                                            # The text goes to stdout and to FILE (default profiles/transcript_ops_bench.txt).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SIZES = (4096, 65536)
CROSS = (16, 64, 256, 1024, 16384)              # 4,096 and 65,536 are rows of the table above
REPS_KERNEL, REPS_CALL = 20, 20


def alternated_ms(f, g, reps):
    """medians of f and g, called in turn"""
    tf, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        g()
        t2 = time.perf_counter()
        tf.append(t1 - t0)
        tg.append(t2 - t1)
    return 1e3 * float(np.median(tf)), 1e3 * float(np.median(tg))


def kernel_ms(eng, f, reps):
    eng.set_profiling(True)
    k = []
    for _ in range(reps):
        f()
        k.append(eng.last_timing()[0]["transcript"])
    eng.set_profiling(False)
    return float(np.median(k))


def routed(eng, T, ts, data, offsets, shared):
    """the route zkp_transcripts_append_message_batch_ctx takes for this batch with the default host_max_terms"""
    eng.set_profiling(True)
    eng.scalar_invert(np.ones((1, 32), np.uint8))                           # (a profiled call of another kind clears the names)
    rc = T.lib().zkp_transcripts_append_message_batch_ctx(eng._h, T._p(ts), len(ts), shared, b"msg", T._p(data), T._p(offsets), 16)
    names = eng.last_kernels().get("transcript", [])
    eng.set_profiling(False)
    assert rc == 0
    return "device" if "zkp::k_strobe_append_csr" in names else "host threads"


def batch(kind, n, rng):
    if kind == "32 B":
        lens = np.full(n, 32)
    elif kind == "0..599 B":
        lens = rng.integers(0, 600, size=n)
    else:
        lens = np.full(n, 4096)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    return rng.integers(0, 256, size=max(int(offsets[-1]), 1), dtype=np.uint8), offsets


def main():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "transcript_ops_bench.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(166)
    eng = Engine(0)
    lib, p = T.lib(), T._p
    t0 = T.Transcript(b"My Sig Application").state
    say("# one MI355X; kernel = HIP events (zkp_ctx_last_timing, kind transcript), median of %d calls; call = the synchronous host-pointer call "
        "zkp_transcripts_append_message / _challenge_bytes, copies included; host = the host threads (zkp_transcripts_append_message_batch, "
        "the parent commit's route) at 16 threads; call and host alternated in one process, median of %d each" % (REPS_KERNEL, REPS_CALL))
    for n in SIZES:
        for kind in ("32 B", "0..599 B", "4096 B"):
            data, offsets = batch(kind, n, rng)
            modes = (("shared", 1),) + ((("in place", 0),) if kind == "0..599 B" else ())
            for mode, shared in modes:
                ts = np.stack([t0] * n)
                dev = lambda: eng.transcripts_append_message(ts, b"msg", data, offsets, shared_initial=bool(shared))                # noqa: E731
                host = lambda: lib.zkp_transcripts_append_message_batch(p(ts), n, shared, b"msg", p(data), p(offsets), 16)         # noqa: E731
                for _ in range(2):                                          # warm: workspace, code objects, thread start, page faults
                    dev()
                    host()
                km = kernel_ms(eng, dev, REPS_KERNEL)
                call, th = alternated_ms(dev, host, REPS_CALL)
                say("append %-9s %-8s N = %6d   kernel %8.3f ms = %8.2f M transcripts/s   call %8.3f ms   host 16 threads %8.3f ms   %s; routed to the %s"
                    % (kind, mode, n, km, n / km / 1e3, call, th, "device call faster" if call < th else "host threads faster",
                       routed(eng, T, ts, data, offsets, shared)))
        ts = lib_ts = np.stack([t0] * n)
        dev = lambda: eng.transcripts_challenge_bytes(ts, b"output", 64)                                                            # noqa: E731
        out = np.zeros((n, 64), np.uint8)
        host = lambda: lib.zkp_transcripts_challenge_bytes_batch(None, p(lib_ts), n, b"output", 64, 16, p(out))                     # noqa: E731
        for _ in range(2):
            dev()
            host()
        km = kernel_ms(eng, dev, REPS_KERNEL)
        call, th = alternated_ms(dev, host, REPS_CALL)
        say("challenge_bytes 64 B       N = %6d   kernel %8.3f ms = %8.2f M transcripts/s   call %8.3f ms   host 16 threads %8.3f ms   %s"
            % (n, km, n / km / 1e3, call, th, "device call faster" if call < th else "host threads faster"))
    say("# crossover, 32-byte messages, shared initial blob: the synchronous device call against the host threads at 16 threads "
        "(alternated, median of %d each)" % REPS_KERNEL)
    for n in CROSS:
        data, offsets = batch("32 B", n, rng)
        ts = np.stack([t0] * n)
        dev = lambda: eng.transcripts_append_message(ts, b"msg", data, offsets, shared_initial=True)                               # noqa: E731
        host = lambda: lib.zkp_transcripts_append_message_batch(p(ts), n, 1, b"msg", p(data), p(offsets), 16)                      # noqa: E731
        for _ in range(2):
            dev()
            host()
        td, th = alternated_ms(dev, host, REPS_CALL)
        say("append 32 B  N = %6d   device call %8.3f ms   host threads %8.3f ms   routed to the %s" % (n, td, th, routed(eng, T, ts, data, offsets, 1)))
    say("# default routing (host_max_terms = %d): an append goes to the device above host_max_terms transcripts when its messages hold 128 bytes or "
        "more per transcript on average; challenge_bytes above host_max_terms transcripts" % T.get_host_max_terms())
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The batched witness RNG, challenge scalars and point appends (zkp_mi355x.h (7)) on one MI355X against the host threads: what the
toolbox's minimum batches (zkp_toolbox_get_witness_rng_min_batch, _challenge_scalars_min_batch, _append_points_min_batch) follow from.

    python tools/transcript_rng_bench.py [--out FILE]   # N = 64, 256, 4,096 and 65,536 transcripts; witness shapes (m, wlen) = (1, 32) and
                                            # (11, 32) with 1 and 11 scalars out; get_challenge; a validating point append.  Per case:
                                            # kernel time from HIP events (zkp_ctx_last_timing, kind transcript), and five rounds in one
                                            # process, each the median of 7 synchronous device calls (copies included) and 7 calls of the
                                            # host route at 16 threads, the two routes alternated call by call.  A route is AHEAD when its
                                            # slowest round beats the other's fastest.  The last lines apply the toolbox's rule: the
                                            # smallest measured N from which the device call is ahead at every measured shape, or never.
                                            # The text goes to stdout and to FILE (default profiles/transcript_rng_bench.txt).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SIZES = (64, 256, 4096, 65536)
SHAPES = ((1, 32), (11, 32))
COUNTS = (1, 11)
ROUNDS, REPS = 5, 7


def rounds_ms(dev, host):
    """ROUNDS x (median of REPS device calls, median of REPS host calls), the routes alternated"""
    out = []
    for _ in range(ROUNDS):
        td, th = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            dev()
            t1 = time.perf_counter()
            host()
            t2 = time.perf_counter()
            td.append(t1 - t0)
            th.append(t2 - t1)
        out.append((1e3 * float(np.median(td)), 1e3 * float(np.median(th))))
    return [r[0] for r in out], [r[1] for r in out]


def kernel_ms(eng, f):
    eng.set_profiling(True)
    k = []
    for _ in range(REPS):
        f()
        k.append(eng.last_timing()[0]["transcript"])
    eng.set_profiling(False)
    return float(np.median(k))


def verdict(d, h):
    if max(d) < min(h):
        return "device AHEAD"
    if max(h) < min(d):
        return "host AHEAD"
    return "within the spread"


def rule(wins):
    """wins: {N: every shape at N has the device ahead} -> the smallest measured N from which the device is ahead at every measured N"""
    best = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        best = n
    return best


def main():
    from zkp_amd import toolbox as T
    from zkp_amd.engine import ZKP_RNG_SCALARS, Engine
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "transcript_rng_bench.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(167)
    eng = Engine(0)
    lib, p = T.lib(), T._p
    t0 = T.Transcript(b"transcript rng bench")
    t0.append_message(b"stmt", bytes(100))
    say("# one MI355X; kernel = HIP events (zkp_ctx_last_timing, kind transcript), median of %d calls; device = the synchronous host-pointer call, "
        "copies included; host = the host route (ctx == NULL) at 16 threads; %d rounds, each the median of %d calls per route, routes alternated; "
        "ms as min .. max over the rounds" % (REPS, ROUNDS, REPS))
    wins = {"witness_rng": {}, "challenge_scalars": {}, "append_points": {}}

    def case(what, text, n, dev, host):
        for _ in range(2):                                                  # warm: workspace, code objects, thread start, page faults
            dev()
            host()
        km = kernel_ms(eng, dev)
        d, h = rounds_ms(dev, host)
        v = verdict(d, h)
        wins[what][n] = wins[what].get(n, True) and v == "device AHEAD"
        say("%-34s N = %6d   kernel %8.3f ms = %8.2f M/s   device %8.3f .. %8.3f ms   host 16 threads %8.3f .. %8.3f ms   %s"
            % (text, n, km, n / km / 1e3, min(d), max(d), min(h), max(h), v))

    for n in SIZES:
        ts = np.stack([t0.state] * n)
        ent = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        for m, wlen in SHAPES:
            wit = rng.integers(0, 256, size=(n, m, wlen), dtype=np.uint8)
            for count in COUNTS:
                out = np.zeros((n, count, 32), np.uint8)
                dev = lambda: eng.transcripts_witness_rng(ts, b"", wit, ent, ZKP_RNG_SCALARS, count)                               # noqa: E731
                host = lambda: lib.zkp_transcripts_witness_rng_batch(None, p(ts), n, b"", m, wlen, p(wit), p(ent), 0, count, 16, p(out))   # noqa: E731
                case("witness_rng", "witness_rng (%2d, %d) -> %2d scalars" % (m, wlen, count), n, dev, host)
        sc = np.zeros((n, 32), np.uint8)
        dev = lambda: eng.transcripts_challenge_scalars(ts, b"chal")                                                                # noqa: E731
        host = lambda: lib.zkp_transcripts_challenge_scalars_batch(None, p(ts), n, b"chal", 16, p(sc))                              # noqa: E731
        case("challenge_scalars", "challenge_scalars", n, dev, host)
        pts = rng.integers(1, 256, size=(n, 32), dtype=np.uint8)
        st = np.zeros(n, np.uint8)
        dev = lambda: eng.transcripts_append_points(ts, b"ptvar", b"C_1", pts, True)                                                # noqa: E731
        host = lambda: lib.zkp_transcripts_append_points_batch(None, p(ts), n, b"ptvar", b"C_1", p(pts), 1, 16, p(st))              # noqa: E731
        case("append_points", "append_points (validate)", n, dev, host)
    say("# the toolbox's rule: the smallest measured N from which the synchronous device call is AHEAD of the host route at 16 threads at every "
        "measured shape; none: never")
    for what in ("witness_rng", "challenge_scalars", "append_points"):
        best = rule(wins[what])
        say("rule: %-18s min_batch = %s   (library default: %s)"
            % (what, "never" if best is None else str(best),
               (lambda v: "never" if v == 2**32 - 1 else str(v))(getattr(T, "get_%s_min_batch" % what)())))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

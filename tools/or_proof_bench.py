#!/usr/bin/env python3
"""The batched 1-of-k OR-proofs (zkp_or_mi355x.h, zkp_or_toolbox.h) on one MI355X against the host backend and against the route callers
had before: what the default of zkp_toolbox_get_or_min_batch follows from.

    python tools/or_proof_bench.py [--out FILE]   # exponential-ElGamal ballots with the DLEQ statement of examples/vote_1_of_k_batch.py.
                                            # k = 2 at N = 4,096 and 65,536 against examples/or_ballot_batch.py's prove and verify on the
                                            # same ballots; k = 4 at both sizes and k = 16 at 4,096 of the new call alone.  Per case and
                                            # for prove and verify: the stream time of the _dev form between HIP events
                                            # (zkp_ctx_last_timing's total), and five rounds in one process of the synchronous device call
                                            # (copies included) and the host backend at 16 threads, the routes alternated call by call,
                                            # min / median / max over the rounds.  A route is AHEAD when its slowest round beats the
                                            # other's fastest.  The last lines apply the toolbox's rule: the smallest measured N from which
                                            # the device call is ahead of the host backend at every measured shape, or never.
                                            # The text goes to stdout and to FILE (default profiles/or_proof_bench.txt).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np

SHAPES = ((2, 4096), (2, 65536), (4, 4096), (4, 65536), (16, 4096))
ROUNDS = 5
NEVER = 2**32 - 1


def rounds_ms(routes):
    """ROUNDS x one call of every route in turn -> {route: [ms per round]}"""
    out = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, f in routes:
            t0 = time.perf_counter()
            f()
            out[name].append(1e3 * (time.perf_counter() - t0))
    return out


def mmm(v):
    return "%9.2f / %9.2f / %9.2f ms" % (min(v), float(np.median(v)), max(v))


def verdict(d, h):
    if max(d) < min(h):
        return "device AHEAD"
    if max(h) < min(d):
        return "host AHEAD"
    return "within the spread"


def main():
    import torch
    torch.cuda.init()
    import or_ballot_batch as OLD
    import vote_1_of_k_batch as V
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine, FusedStatement
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "or_proof_bench.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = Engine(0)
    st = V.statement()
    fst = FusedStatement(st.proof_label, st.secrets, st.points, st.constraints)
    say("# one MI355X; stream = the _dev form between HIP events on the context's stream (zkp_ctx_last_timing, total), median of %d calls; device = the "
        "synchronous call through the toolbox (threshold 0), copies included; host = the host backend (ctx == NULL) at 16 threads; old = "
        "examples/or_ballot_batch.py's prove / verify on the same ballots with the engine (k = 2 only); %d rounds, one call per route and round, routes "
        "alternated; min / median / max over the rounds" % (ROUNDS, ROUNDS))
    wins = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")        # noqa: E731
    for k, n in SHAPES:
        rng = np.random.default_rng(n + k)
        votes = rng.integers(0, k, size=n)
        secrets = T.scalar_random(eng, n + 1, bytes(range(32)))
        y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
        Y = T.basepoint_mul(eng, y)[0]
        common = np.stack([V.BASEPOINT, Y])
        C1, C2 = V.encrypt(eng, Y, r, votes)
        inst = V.branch_points(eng, C1, C2, k)
        ent = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sec, real, ts0 = r.reshape(n, 1, 32), votes.astype(np.uint8), V.transcripts(n)
        T.set_or_min_batch(0)
        chal, resp, status = T.or_prove(eng, st, ts0.copy(), sec, real, inst, common, ent)
        assert not status.any() and not T.or_verify(eng, st, ts0.copy(), inst, common, chal, resp).any()

        def route(e, what):
            if what == "prove":
                return lambda: T.or_prove(e, st, ts0.copy(), sec, real, inst, common, ent, 16)
            return lambda: T.or_verify(e, st, ts0.copy(), inst, common, chal, resp, 16)

        # the _dev forms: stream time
        d = {name: dev(a) for name, a in (("sec", sec), ("real", real), ("inst", inst), ("common", common), ("ent", ent), ("chal", chal), ("resp", resp))}
        d_ts, d_status = dev(ts0), torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        stream = {"prove": [], "verify": []}
        eng.set_profiling(True)
        for _ in range(ROUNDS + 1):
            d_ts.copy_(torch.from_numpy(ts0))
            torch.cuda.synchronize()
            eng.or_prove_dev(fst, k, n, d_ts.data_ptr(), d["sec"].data_ptr(), d["real"].data_ptr(), d["inst"].data_ptr(), d["common"].data_ptr(),
                             d["ent"].data_ptr(), d["chal"].data_ptr(), d["resp"].data_ptr(), d_status.data_ptr())
            eng.synchronize()
            stream["prove"].append(eng.last_timing()[1])
            d_ts.copy_(torch.from_numpy(ts0))
            torch.cuda.synchronize()
            eng.or_verify_dev(fst, k, n, d_ts.data_ptr(), d["inst"].data_ptr(), d["common"].data_ptr(), d["chal"].data_ptr(), d["resp"].data_ptr(),
                              d_status.data_ptr())
            eng.synchronize()
            stream["verify"].append(eng.last_timing()[1])
        eng.set_profiling(False)
        assert not d_status.cpu().numpy().any()
        for what in ("prove", "verify"):
            routes = [("device", route(eng, what)), ("host", route(None, what))]
            if k == 2:
                Ys = Y.reshape(1, 32)
                if what == "prove":
                    routes.append(("old", lambda: OLD.prove(eng, Ys, C1, C2, r, votes, ent)))
                else:
                    old_proof = OLD.prove(eng, Ys, C1, C2, r, votes, ent)
                    assert OLD.verify(eng, Ys, C1, C2, old_proof).all()
                    routes.append(("old", lambda: OLD.verify(eng, Ys, C1, C2, old_proof)))
            for _, f in routes:                                                 # warm: workspace, code objects, thread start, page faults
                f()
            t = rounds_ms(routes)
            v = verdict(t["device"], t["host"])
            wins[n] = wins.get(n, True) and v == "device AHEAD"
            say("%-6s k = %2d N = %6d   stream %9.2f ms   device %s   host 16 threads %s   %s%s"
                % (what, k, n, float(np.median(stream[what][1:])), mmm(t["device"]), mmm(t["host"]), v,
                   ("   old route %s (%s)" % (mmm(t["old"]), "new call ahead" if max(t["device"]) < min(t["old"]) else
                                              "old route ahead" if max(t["old"]) < min(t["device"]) else "within the spread")) if "old" in t else ""))
    best = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        best = n
    T.set_or_min_batch(NEVER)
    say("# the toolbox's rule: the smallest measured N from which the synchronous device call is AHEAD of the host backend at 16 threads at every "
        "measured shape; none: never")
    say("rule: or_min_batch = %s" % ("never" if best is None else str(best)))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

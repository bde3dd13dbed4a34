#!/usr/bin/env python3
"""The batchable 1-of-k OR-proofs (zkp_or_batch_mi355x.h, zkp_or_batch_toolbox.h) on one MI355X: what the batch verifier gains over
zkp_or_verify and over the host backend, what the batchable prover costs over zkp_or_prove, and what the default of
zkp_toolbox_get_or_batch_min_batch follows from.

    python tools/or_batch_bench.py [--out FILE] [--parent-tree DIR]
        exponential-ElGamal ballots with the DLEQ statement of examples/vote_1_of_k_batch.py; (k, N) = (2, 4096), (2, 65536), (4, 4096),
        (4, 65536), (16, 4096).  Per shape, five rounds in one process, the routes alternated call by call, min / median / max:
          verify   the synchronous zkp_or_batch_verify (copies included) | zkp_or_verify on the same proofs | the host backend's batch
                   check at 16 threads; and the stream time of zkp_or_batch_verify_dev and zkp_or_verify_dev between HIP events
          prove    the synchronous zkp_or_prove_batchable | zkp_or_prove
        A route is AHEAD when its slowest round beats the other's fastest.  The last lines apply the toolbox's rule: the smallest measured N
        from which the synchronous batch check is AHEAD of the host backend at every measured shape, or never.
        --parent-tree DIR: a checkout of the parent commit with its libraries built.  zkp_or_prove and zkp_or_verify are then measured at
        (2, 4096) and (2, 65536) from this tree and from DIR in child processes of their own, alternated, before this process opens the GPU.
        The text goes to stdout and to FILE (default profiles/or_batch_verify_bench.txt).
    python tools/or_batch_bench.py --existing --tree DIR      (what the child processes run: the rounds as one JSON line)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 4096), (2, 65536), (4, 4096), (4, 65536), (16, 4096))
EXISTING_SHAPES = ((2, 4096), (2, 65536))
ROUNDS = 5
NEVER = 2**32 - 1


def mmm(v):
    return "%9.2f / %9.2f / %9.2f ms" % (min(v), sorted(v)[len(v) // 2], max(v))


def ahead(a, b, name_a, name_b):
    if max(a) < min(b):
        return "%s AHEAD" % name_a
    if max(b) < min(a):
        return "%s AHEAD" % name_b
    return "within the spread"


def rounds_ms(routes):
    """ROUNDS x one call of every route in turn -> {route: [ms per round]}"""
    out = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, f in routes:
            t0 = time.perf_counter()
            f()
            out[name].append(1e3 * (time.perf_counter() - t0))
    return out


def ballots(T, V, eng, k, n):
    import numpy as np
    rng = np.random.default_rng(n + k)
    votes = rng.integers(0, k, size=n)
    secrets = T.scalar_random(eng, n + 1, bytes(range(32)))
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)[0]
    common = np.stack([V.BASEPOINT, Y])
    C1, C2 = V.encrypt(eng, Y, r, votes)
    inst = V.branch_points(eng, C1, C2, k)
    ent = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    return r.reshape(n, 1, 32), votes.astype(np.uint8), inst, common, ent, V.transcripts(n)


def existing(tree):
    """zkp_or_prove / zkp_or_verify as synchronous calls from the tree at `tree`: {"prove k N": [ms], "verify k N": [ms]} as one JSON line"""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "examples"))
    import torch
    torch.cuda.init()
    import vote_1_of_k_batch as V
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    eng = Engine(0)
    T.set_or_min_batch(0)
    out = {}
    for k, n in EXISTING_SHAPES:
        sec, real, inst, common, ent, ts0 = ballots(T, V, eng, k, n)
        chal, resp, status = T.or_prove(eng, V.statement(), ts0.copy(), sec, real, inst, common, ent)
        st = V.statement()
        routes = [("prove %d %d" % (k, n), lambda: T.or_prove(eng, st, ts0.copy(), sec, real, inst, common, ent)),
                  ("verify %d %d" % (k, n), lambda: T.or_verify(eng, st, ts0.copy(), inst, common, chal, resp))]
        for _, f in routes:
            f()
        out.update(rounds_ms(routes))
    eng.close()
    print(json.dumps(out))


def main():
    if "--existing" in sys.argv:
        existing(sys.argv[sys.argv.index("--tree") + 1])
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "or_batch_verify_bench.txt")
    parent = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the existing calls against the parent commit: child processes of their own, alternated, before this process opens the GPU
    old = {}
    if parent:
        for _ in range(2):
            for name, tree in (("this", ROOT), ("parent", os.path.abspath(parent))):
                r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--existing", "--tree", tree], capture_output=True,
                                   text=True, check=True)
                for key, v in json.loads(r.stdout.strip().split("\n")[-1]).items():
                    old.setdefault((key, name), []).extend(v)

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import numpy as np
    import torch
    torch.cuda.init()
    import vote_1_of_k_batch as V
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine, FusedStatement
    eng = Engine(0)
    st = V.statement()
    fst = FusedStatement(st.proof_label, st.secrets, st.points, st.constraints)
    say("# one MI355X; DLEQ ballots (ns 2, ni 2, nc 2: the batch sum has 2 + 4 N k operands); batch = the synchronous zkp_or_batch_verify through the "
        "toolbox (threshold 0), copies included; each = zkp_or_verify on the same proofs, likewise; host = the host backend's batch check (ctx == NULL) "
        "at 16 threads; stream = the _dev forms between HIP events on the context's stream (zkp_ctx_last_timing, total), median of %d calls; %d rounds, "
        "one call per route and round, routes alternated; min / median / max over the rounds" % (ROUNDS, ROUNDS))
    T.set_or_min_batch(0)
    T.set_or_batch_min_batch(0)
    wins = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")        # noqa: E731
    for k, n in SHAPES:
        sec, real, inst, common, ent, ts0 = ballots(T, V, eng, k, n)
        coms, chal, resp, status = T.or_prove_batchable(eng, st, ts0.copy(), sec, real, inst, common, ent)
        w = np.random.default_rng(n).integers(0, 256, size=(n, k, 2, 16), dtype=np.uint8)
        assert not status.any() and T.or_batch_verify(eng, st, ts0.copy(), inst, common, coms, chal, resp, w)
        assert not T.or_verify(eng, st, ts0.copy(), inst, common, chal, resp).any()

        d = {name: dev(a) for name, a in (("inst", inst), ("common", common), ("coms", coms), ("chal", chal), ("resp", resp), ("w", w))}
        d_ts, d_res, d_verdict = dev(ts0), torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.ones(1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        stream = {"batch": [], "each": []}
        eng.set_profiling(True)
        for _ in range(ROUNDS + 1):
            d_ts.copy_(torch.from_numpy(ts0))
            torch.cuda.synchronize()
            eng.or_batch_verify_dev(fst, k, n, d_ts.data_ptr(), d["inst"].data_ptr(), d["common"].data_ptr(), d["coms"].data_ptr(), d["chal"].data_ptr(),
                                    d["resp"].data_ptr(), d["w"].data_ptr(), d_verdict.data_ptr())
            eng.synchronize()
            stream["batch"].append(eng.last_timing()[1])
            d_ts.copy_(torch.from_numpy(ts0))
            torch.cuda.synchronize()
            eng.or_verify_dev(fst, k, n, d_ts.data_ptr(), d["inst"].data_ptr(), d["common"].data_ptr(), d["chal"].data_ptr(), d["resp"].data_ptr(), d_res.data_ptr())
            eng.synchronize()
            stream["each"].append(eng.last_timing()[1])
        eng.set_profiling(False)
        assert int(d_verdict.cpu().numpy()[0]) == 0 and not d_res.cpu().numpy().any()

        routes = [("batch", lambda: T.or_batch_verify(eng, st, ts0.copy(), inst, common, coms, chal, resp, w)),
                  ("each", lambda: T.or_verify(eng, st, ts0.copy(), inst, common, chal, resp)),
                  ("host", lambda: T.or_batch_verify(None, st, ts0.copy(), inst, common, coms, chal, resp, w, 16))]
        for _, f in routes:                                                     # warm: workspace, code objects, thread start, page faults
            f()
        t = rounds_ms(routes)
        v_host = ahead(t["batch"], t["host"], "device", "host")
        wins[n] = wins.get(n, True) and v_host == "device AHEAD"
        say("verify k = %2d N = %6d   batch %s   each %s   %s   host 16 threads %s   %s   stream: batch %8.2f ms, each %8.2f ms"
            % (k, n, mmm(t["batch"]), mmm(t["each"]), ahead(t["batch"], t["each"], "batch", "each"), mmm(t["host"]), v_host,
               float(np.median(stream["batch"][1:])), float(np.median(stream["each"][1:]))))
        routes = [("batchable", lambda: T.or_prove_batchable(eng, st, ts0.copy(), sec, real, inst, common, ent)),
                  ("plain", lambda: T.or_prove(eng, st, ts0.copy(), sec, real, inst, common, ent))]
        for _, f in routes:
            f()
        t = rounds_ms(routes)
        say("prove  k = %2d N = %6d   zkp_or_prove_batchable %s   zkp_or_prove %s   %s"
            % (k, n, mmm(t["batchable"]), mmm(t["plain"]), ahead(t["batchable"], t["plain"], "batchable", "plain")))
    if old:
        say("# the existing calls against a library built from the parent commit: synchronous calls, a process of its own per library, two processes "
            "each, alternated, %d rounds per process" % ROUNDS)
        for key in sorted({key for key, _ in old}):
            what, k, n = key.split()
            a, b = old[(key, "this")], old[(key, "parent")]
            say("zkp_or_%-6s k = %2d N = %6d   this tree %s   parent %s   %s" % (what, int(k), int(n), mmm(a), mmm(b), ahead(a, b, "this tree", "parent")))
    best = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        best = n
    say("# the toolbox's rule: the smallest measured N from which the synchronous batch check is AHEAD of the host backend at 16 threads at every "
        "measured shape; none: never")
    say("rule: or_batch_min_batch = %s" % ("never" if best is None else str(best)))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

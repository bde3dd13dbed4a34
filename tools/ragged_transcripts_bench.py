#!/usr/bin/env python3
"""Ragged transcript batches (zkp_fused_*_ragged, k_transcript_run_ragged) on one MI355X: what a batch of signatures over messages of
different lengths costs on the device, against the same batch with aligned transcripts and against the host-transcript route.

    python tools/ragged_transcripts_bench.py [--out profiles/ragged_transcripts_bench.txt] [--sizes 4096,65536] [--reps 7]
    rocprofv3 --kernel-trace --stats -d OUT -o ragged -- python tools/ragged_transcripts_bench.py --trace     # one ragged call per flow

For the sig statement (sig_and_vrf_example.rs: A = x * B) and the CMZ statement (benches/zkp.rs cred_show_10), at each size, three cases:
aligned (every message 100 bytes: one STROBE position, zkp_fused_*), ragged (lengths 0..599: up to 166 positions, the _ragged calls) and
ragged on the host route (set_fused_min_batch(NEVER): host Merlin, device MSMs).  Every call runs on transcripts over fresh random messages.
Per flow (prove, verify_compact, batch_verify) the median wall time of synchronous toolbox calls after warm-up (host clock around a call that
ends in a device synchronise), the device time of the call's kernels and the job's stream span (a separate profiled call), and the cost of
the first ragged call on a new context, which compiles the base plan and every class program."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

NEVER = 0xFFFFFFFF
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


def _rs(rng, k):
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def sig_inputs(eng, n, rng):
    from zkp_amd import toolbox as T
    from zkp_amd.engine import ZKP_CT
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    x = _rs(rng, n)
    A, _ = eng.msm_many(np.arange(n + 1, dtype=np.uint32), x, np.zeros(n, np.uint32), B, ZKP_CT)
    st = T.define_proof("sig_proof", b"Sig", ["x"], ["A"], ["B"], [("A", [("x", "B")])]).statement
    return st, x.reshape(n, 1, 32), np.ascontiguousarray(A[None]), B


def cmz_inputs(eng, n, rng):
    """n CMZ presentations (C_i = m_i P + z_i A, V = sum m_i X_i + minus_z_Q Q), made by the engine's own MSM; 4096 distinct ones, tiled"""
    from zkp_amd import toolbox as T
    from zkp_amd.engine import ZKP_CT
    k = min(n, 4096)
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    iota = lambda m: np.arange(m + 1, dtype=np.uint32)
    common, _ = eng.msm_many(iota(12), _rs(rng, 12), np.zeros(12, np.uint32), B, ZKP_CT)              # X_1..X_10, A, B
    secrets = _rs(rng, k * 21).reshape(k, 21, 32)
    pq, _ = eng.msm_many(iota(2 * k), _rs(rng, 2 * k), np.zeros(2 * k, np.uint32), B, ZKP_CT)
    table = np.concatenate([common, pq])
    off, scal, pidx = [0], [], []
    for j in range(k):
        for i in range(10):
            scal += [secrets[j, i], secrets[j, 10 + i]]
            pidx += [12 + j, 10]
            off.append(len(pidx))
        for i in range(10):
            scal.append(secrets[j, i]); pidx.append(i)
        scal.append(secrets[j, 20]); pidx.append(12 + k + j)
        off.append(len(pidx))
    cv, _ = eng.msm_many(np.array(off, np.uint32), np.stack(scal), np.array(pidx, np.uint32), table, ZKP_CT)
    cv = cv.reshape(k, 11, 32)
    inst = np.concatenate([cv[:, :10].transpose(1, 0, 2), pq[None, :k], pq[None, k:], cv[:, 10][None]])
    reps = (n + k - 1) // k
    secrets = np.tile(secrets, (reps, 1, 1))[:n]
    inst = np.ascontiguousarray(np.tile(inst, (1, reps, 1))[:, :n])
    return T.cmz_module(10).statement, secrets, inst, common


def transcripts(n, ragged, rng):
    from zkp_amd import toolbox as T
    lens = rng.integers(0, 600, size=n) if ragged else np.full(n, 100)
    return T.append_messages(b"bench", b"msg", [rng.bytes(int(k)) for k in lens])


def job_ms(eng):
    """(copies in, kernels, copies out) of the context's last host-buffer job (zkp_ctx_job_timing; profiling on)"""
    import ctypes
    ms = (ctypes.c_float * 3)()
    eng._lib.zkp_ctx_job_timing(eng._h, ms)
    return list(ms)


def run_case(eng, st, secrets, inst, common, n, ragged, route, reps, rng):
    """Every call gets transcripts over fresh random messages (its own STROBE positions); the proofs a timed prove made are what the
    verifiers then check.  -> {flow: (median wall ms, kernel ms, job ms or None)}"""
    from zkp_amd import toolbox as T
    T.set_fused_min_batch(NEVER if route == "host" else 32)
    w = rng.integers(0, 256, size=(st.nc, n, 16), dtype=np.uint8)
    wall = {"prove": [], "verify_compact": [], "batch_verify": []}
    prof = {}
    for k in range(reps + 3):                 # 2 warm-up sets, reps timed sets, 1 profiled set
        ts0 = transcripts(n, ragged, rng)
        entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        profiled = k == reps + 2
        if profiled:
            eng.set_profiling(True)
        calls = {}
        ts = ts0.copy()
        t0 = time.perf_counter()
        chal, resp, coms = T.prove_batch(eng, st, ts, secrets, inst, common, entropy)
        calls["prove"] = time.perf_counter() - t0
        if profiled:
            prof["prove"] = (eng.last_timing()[1], job_ms(eng))
        ts = ts0.copy()
        t0 = time.perf_counter()
        T.verify_compact_batch(eng, st, ts, inst, common, chal, resp)
        calls["verify_compact"] = time.perf_counter() - t0
        if profiled:
            prof["verify_compact"] = (eng.last_timing()[1], job_ms(eng))
        ts = ts0.copy()
        t0 = time.perf_counter()
        T.batch_verify(eng, st, ts, inst, common, coms, resp, w)
        calls["batch_verify"] = time.perf_counter() - t0
        if profiled:
            prof["batch_verify"] = (eng.last_timing()[1], job_ms(eng))
            eng.set_profiling(False)
        elif k >= 2:
            for f, t in calls.items():
                wall[f].append(1e3 * t)
    T.set_fused_min_batch(32)
    return {f: (float(np.median(wall[f])), float(prof[f][0]), None if route == "host" else sum(prof[f][1])) for f in wall}


def cold_calls(st_maker, n, rng):
    """wall ms of the first ragged prove on a new context (every class program and the base plan compiled) and of the next one"""
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    e = Engine(0)
    st, secrets, inst, common = st_maker(e, n, rng)
    out = []
    for _ in range(2):
        ts = transcripts(n, True, rng)
        entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        t0 = time.perf_counter()
        T.prove_batch(e, st, ts, secrets, inst, common, entropy)
        out.append(1e3 * (time.perf_counter() - t0))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_transcripts_bench.txt"))
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="one ragged prove / verify_compact / batch_verify of 4096 sig proofs, for rocprofv3")
    a = ap.parse_args()
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(1)
    if a.trace:
        st, x, inst, common = sig_inputs(eng, 4096, rng)
        run_case(eng, st, x, inst, common, 4096, True, "device", 1, rng)
        eng.close()
        return
    lines = ["# tools/ragged_transcripts_bench.py on one MI355X: synchronous toolbox calls, every call on transcripts over fresh random messages.",
             "# wall = median of %d calls after 2 warm-up calls (host clock around a call that ends in a device synchronise); kernel = device time of" % a.reps,
             "# the call's kernels and job = its stream span from the first copy in to the last copy out (zkp_ctx_last_timing / zkp_ctx_job_timing,",
             "# a separate profiled call).  wall - job = host work in front of the job (class grouping, lookups, plan, argument checks).",
             "# aligned: 100-byte messages (one STROBE position); ragged: 0..599-byte messages; host: the ragged batch on the host-transcript route.",
             "%-5s %6s %-14s %-8s %10s %10s %10s" % ("stmt", "N", "flow", "case", "wall_ms", "kernel_ms", "job_ms")]
    st, secrets, inst, common = sig_inputs(eng, 4096, rng)             # process warm-up (first launches, host pools), not recorded
    run_case(eng, st, secrets, inst, common, 4096, False, "device", 2, rng)
    for n in [int(s_) for s_ in a.sizes.split(",")]:
        for stmt, make in (("sig", sig_inputs), ("cmz", cmz_inputs)):
            st, secrets, inst, common = make(eng, n, rng)
            res = {}
            for case, ragged, route in (("aligned", False, "device"), ("ragged", True, "device"), ("host", True, "host")):
                res[case] = run_case(eng, st, secrets, inst, common, n, ragged, route, a.reps, rng)
                for flow, (wall, kern, job) in res[case].items():
                    lines.append("%-5s %6d %-14s %-8s %10.3f %10.3f %10s" % (stmt, n, flow, case, wall, kern, "-" if job is None else "%.3f" % job))
            pb = lambda c: res[c]["prove"][0] + res[c]["batch_verify"][0]
            lines.append("%-5s %6d prove+batch_verify wall: ragged / aligned = %.2f, host / ragged = %.2f" % (stmt, n, pb("ragged") / pb("aligned"), pb("host") / pb("ragged")))
            if n <= 4096:
                cold, warm = cold_calls(make, n, rng)
                lines.append("%-5s %6d ragged prove on a new context: first call %.2f ms (base plan + every class program compiled), next call %.2f ms"
                             % (stmt, n, cold, warm))
            print("\n".join(lines[-12:]), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

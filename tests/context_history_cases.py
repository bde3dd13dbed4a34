"""(helper module of tests/test_host_context_history.py and tests/test_gpu_context_history.py)
One seeded, fixed script of calls for ONE long-lived context, with what every call must return.

A context keeps state across calls -- the grow-only workspace, the aligned plan cache (flushed whole when a 65th plan arrives), the ragged
program and base caches (64 bases, least recently used first out), the 64 fixed-base slots, the option words -- and include/zkp_mi355x.h
promises that none of it changes a result.  The script drives each of those through its interesting transition and says, step by step,
what the call must give.  No expectation comes from the device:

  "oracle"   the C oracle's prover (aligned proofs, byte for byte) and oracle/cbind.msm_many (MSM outputs and statuses)
  "planted"  verdicts: exactly the proofs / batches the script tampered with
  "host"     the host backend of the toolbox (ragged proofs: the C oracle starts every transcript from a label)

Steps are dicts: kind, the call's inputs, `expect`, and for calls that reach the aligned plan cache `key` = (flow, statement, N, position).
build() returns them in order; run_step() replays one step on an engine (zkp_amd.engine.Engine methods on host arrays, so that the
test-hook build can be driven too) or on the toolbox's host backend (eng = None)."""
import numpy as np

from oracle import cbind as C
from oracle import model as M

SEED = 20261018
BASE = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8).reshape(1, 32)
JUNK = np.frombuffer(bytes([1] + [0] * 31), np.uint8)          # not a ristretto255 encoding
LABEL = b"history"
OPT = dict(TRANSCRIPT_LANES=4, FUSE_TABLES_TRANSCRIPT=8, CT_LOOKUP=9, EACH_STRAUS=10, WS_LIMIT_BYTES=12, SYNC_SCHEDULE=14, TRANSCRIPT_STEPS=15,
           COMB_SPLIT=16, JOINT_LADDER=17)
DEFAULT = 2**64 - 1
PLAN_CAP, RAGGED_BASE_CAP, HOT_SLOTS = 64, 64, 64
SMALL_N = 65
# operands a flow touches per proof (terms of its MSMs): what every region of its workspace layout is proportional to.  Used as the
# measure of "a much larger call came first"; the large calls of the script are all CMZ, whose per-proof regions (comb tables of P and Q,
# 21 secrets) are larger per term than DLEQ's, so the measure understates the ratio of the workspace needs.
TERMS = {("prove", "dleq"): 2, ("verify_compact", "dleq"): 4, ("verify_each", "dleq"): 6, ("batch", "dleq"): 5,
         ("prove", "cmz"): 31, ("verify_compact", "cmz"): 42, ("verify_each", "cmz"): 36, ("batch", "cmz"): 24}


class _OracleMsm:
    """stands where bench.make_instance expects an engine: its MSMs by the C oracle"""
    @staticmethod
    def msm_many(off, sc, pidx, pts, flags):
        return C.msm_many(off, sc, pidx, pts, flags)


def _rs(rng, k):
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def _statements():
    import bench
    from zkp_amd import toolbox as T
    return {"dleq": (bench.dleq_macro_statement(), b"DLEQ proof", T.dleq_module().statement, C.Statement.from_model(M.dleq_statement())),
            "cmz": (bench.cmz_statement(), b"CMZ cred show n=10", T.cmz_module().statement, C.Statement.from_model(M.cmz_statement()))}


_CACHE = {}


def fused_statement(which):
    from zkp_amd.engine import FusedStatement
    if ("fst", which) not in _CACHE:
        st, label = _statements()[which][:2]
        _CACHE[("fst", which)] = FusedStatement(label, *st)
    return _CACHE[("fst", which)]


def _aligned(n):
    from zkp_amd import toolbox as T
    t0 = T.Transcript(LABEL).state
    return np.stack([t0] * n), int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16


def _ragged_ts(n, rng):
    """two STROBE position classes, interleaved"""
    from zkp_amd import toolbox as T
    return T.append_messages(LABEL, b"msg", [rng.bytes((11, 97)[j % 2]) for j in range(n)])


def _proofs(which, n, rng, ragged=False):
    """n honest proofs: inputs, and the proofs themselves from the C oracle (aligned) or the host backend (ragged)"""
    import bench
    from zkp_amd import toolbox as T
    st, _, tst, cst = _statements()[which]
    secrets, inst, common = bench.make_instance(_OracleMsm, st, n, rng)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if ragged:
        ts0 = _ragged_ts(n, rng)
        ts = ts0.copy()
        chal, resp, coms = T.prove_batch(T.HostEngine(), tst, ts, secrets, inst, common, entropy)
        pos, source = None, "host"
    else:
        ts0, pos = _aligned(n)
        out = [C.prove(cst, LABEL, secrets[j], np.concatenate([inst[:, j], common]), entropy[j].tobytes())[:3] for j in range(n)]
        chal, resp, coms = (np.stack([o[i] for o in out]) for i in range(3))
        source = "oracle"
    return dict(which=which, n=n, secrets=secrets, inst=inst, common=common, entropy=entropy, ts0=ts0, pos=pos, chal=chal, resp=resp, coms=coms,
                source=source, ragged=ragged)


def _tamper(resp, where):
    bad = resp.copy()
    for j in where:
        bad[j, 0, 0] ^= 1
    return bad


def _step(kind, p, **kw):
    s = dict(kind=kind, which=p["which"], n=p["n"], p=p, ragged=p["ragged"])
    s.update(kw)
    flow = {"prove": "P", "verify_compact": "V", "verify_each": "B", "batch": "B"}[kind]
    s["key"] = None if p["ragged"] else (flow, p["which"], p["n"], p["pos"])
    s["base"] = (flow, p["which"], p["n"]) if p["ragged"] else None
    return s


def prove_step(p):
    return _step("prove", p, expect=(p["chal"], p["resp"], p["coms"]), source=p["source"])


def verify_step(kind, p, mutants, rng, K=1):
    """verify_compact / verify_each: per-proof verdicts = the mutants; batch: K verdicts = the batches that hold a mutant"""
    nc = p["coms"].shape[1]
    n = p["n"]
    if kind == "batch":
        w = rng.integers(0, 256, size=(nc, n, 16), dtype=np.uint8)
        each = n // K
        expect = np.array([int(any(b * each <= j < (b + 1) * each for j in mutants)) for b in range(K)], np.int32)
    else:
        w = rng.integers(0, 256, size=(n, nc, 16), dtype=np.uint8)
        expect = np.zeros(n, np.uint8)
        expect[list(mutants)] = 1
    return _step(kind, p, responses=_tamper(p["resp"], mutants), w=w, K=K, mutants=sorted(mutants), expect=expect, source="planted")


def job_step(p, mutants, rng, mode):
    """zkp_fused_verify_compact_submit, then zkp_ctx_job_wait (verdicts = the mutants) or zkp_ctx_job_discard (no copy out: the verdict words
    stay as submit poisoned them, every proof rejected)"""
    s = verify_step("verify_compact", p, mutants, rng)
    s.update(kind="job", mode=mode)
    if mode == "discard":
        s.update(expect=np.ones(p["n"], np.uint8), verdicts_if_waited=s["expect"])
    return s


def small_after_large(S):
    """indices i of calls at N <= SMALL_N that come right after a call of a DIFFERENT flow touching at least 8 times as many operands"""
    calls = ("prove", "verify_compact", "verify_each", "batch")
    out = []
    for i in range(1, len(S)):
        prev, cur = S[i - 1], S[i]
        if cur["kind"] in calls and prev["kind"] in calls and prev["kind"] != cur["kind"] and cur["n"] <= SMALL_N and \
                prev["n"] * TERMS[(prev["kind"], prev["which"])] >= 8 * cur["n"] * TERMS[(cur["kind"], cur["which"])]:
            out.append(i)
    return out


def msm_step(points, logs_unused, rng, flags, n_terms=96):
    """a small CSR job over `points` (the CMZ common points: registered, evicted, unregistered or registered again -- same outputs)"""
    off = np.arange(0, n_terms + 1, 3, dtype=np.uint32)
    sc = _rs(rng, n_terms)
    pidx = rng.integers(0, len(points), size=n_terms).astype(np.uint32)
    out, st = C.msm_many(off, sc, pidx, points, flags)
    return dict(kind="msm_many", off=off, sc=sc, pidx=pidx, points=points, flags=flags, expect=(out, st), source="oracle", key=None, base=None, n=len(off) - 1)


def option_step(name, value, refused=False):
    return dict(kind="option", option=OPT[name], name=name, value=value, refused=refused, key=None, base=None)


def build():
    """-> the list of steps (built once per process)"""
    if "script" in _CACHE:
        return _CACHE["script"]
    rng = np.random.default_rng(SEED)
    S = []
    dleq = {n: _proofs("dleq", n, rng) for n in range(1, 71)}
    cmz_big, cmz_mid = _proofs("cmz", 256, rng), _proofs("cmz", 64, rng)
    common = cmz_mid["common"]                     # the common points of the CMZ proofs that part 4 proves between registrations

    # ---- 1. sizes go down after they went up: a large CMZ call, then another flow at a small N ----------------------------------------
    S.append(prove_step(cmz_big))
    S.append(verify_step("verify_compact", dleq[5], {0, 4}, rng))
    S.append(verify_step("batch", cmz_big, {130}, rng, K=2))
    S.append(prove_step(dleq[3]))
    S.append(verify_step("verify_each", cmz_big, {0, 255}, rng))
    S.append(verify_step("batch", dleq[4], set(), rng))
    S.append(verify_step("batch", dleq[8], set(), rng))               # (its plan is the one the captured graph of part 5 replays)
    S.append(verify_step("verify_compact", cmz_big, {63, 64, 255}, rng))
    S.append(verify_step("verify_each", dleq[7], {6}, rng))

    # ---- 2. reject / accept alternation at two sizes per verify flow, another flow between each pair -----------------------------------
    for kind in ("verify_compact", "verify_each", "batch"):
        for n in (9, 65):
            for k, mut in enumerate(({0, n - 1}, set(), {n // 2}, set())):
                S.append(verify_step(kind, dleq[n], mut, rng))
                if k < 3:
                    S.append(prove_step(dleq[2]) if kind != "verify_compact" else verify_step("verify_each", dleq[2], {1}, rng))

    # ---- 2b. a host-buffer job between synchronous calls: submitted and waited for, then submitted and discarded ---------------------------
    S.append(prove_step(dleq[2]))
    S.append(job_step(dleq[12], {0, 11}, rng, "wait"))
    S.append(verify_step("verify_each", dleq[2], {1}, rng))
    S.append(job_step(dleq[12], {0, 11}, rng, "discard"))                 # its verdict words keep what submit put there: rejected, all of them
    S.append(verify_step("verify_compact", dleq[12], {5}, rng))           # the same flow at the same size right behind the discarded job

    # ---- 3. options flipped on a context whose plans are cached: the same flow at the same N between flips ------------------------------
    def flips(name, values, probe, refused=()):
        S.append(probe())
        for v in values:
            S.append(option_step(name, v, refused=v in refused))
            S.append(probe())
    flips("JOINT_LADDER", (0, 2, 1), lambda: verify_step("verify_compact", cmz_mid, {0, 63}, np.random.default_rng(1)))
    flips("TRANSCRIPT_STEPS", (0, 1), lambda: prove_step(cmz_mid))
    flips("TRANSCRIPT_LANES", (1, 2, DEFAULT), lambda: prove_step(dleq[33]))
    flips("FUSE_TABLES_TRANSCRIPT", (0, 1, 2, 0, DEFAULT), lambda: prove_step(cmz_mid))
    flips("COMB_SPLIT", (0, 1, 2, 0, DEFAULT), lambda: prove_step(cmz_mid))
    flips("EACH_STRAUS", (0, 1, 2, 0, DEFAULT), lambda: verify_step("verify_each", dleq[40], {0, 39}, np.random.default_rng(2)))
    flips("CT_LOOKUP", (0, 1, 2, 0), lambda: prove_step(cmz_mid), refused=(1, 2))     # masked scans / LDS rows exist in 6-bit-window builds only: refused, nothing changes
    flips("SYNC_SCHEDULE", (1, 0), lambda: prove_step(cmz_mid))

    # ---- 4. fixed-base slots: the CMZ common points registered, evicted by others, used unregistered, registered again ------------------
    other, _ = C.msm_many(np.arange(127, dtype=np.uint32), _rs(rng, 126), np.zeros(126, np.uint32), BASE, 0)
    batches = [common, other[:64], np.concatenate([other[64:96], JUNK[None], np.zeros((1, 32), np.uint8), other[96:126]]), common]
    for enc in batches:
        S.append(dict(kind="register", encodings=np.ascontiguousarray(enc), key=None, base=None))
        S.append(msm_step(common, None, np.random.default_rng(3), 1))
        S.append(msm_step(common, None, np.random.default_rng(3), 0))
        S.append(prove_step(cmz_mid))

    # ---- 5. the plan cache: DLEQ prove at N = 1 .. 70; the cache is flushed when its 65th plan arrives --------------------------------
    S.append(dict(kind="ragged_probe", key=None, base=None))               # (test-hook context: reports the size of the plan cache)
    first_plan = S[0]
    keys = []
    for s in S:
        if s.get("key") and s["key"] not in keys:
            keys.append(s["key"])
    for n in range(1, 71):
        s = prove_step(dleq[n])
        if s["key"] not in keys:
            if len(keys) == PLAN_CAP:
                S.append(dict(kind="graph_capture", p=dleq[8], key=None, base=None))      # just before the plan that flushes the cache (GPU only)
                s["flushes"] = True
            keys.append(s["key"])
        S.append(s)
        if s.get("flushes"):
            S.append(dict(kind="graph_stale", key=None, base=None))
            S.append(dict(kind="ragged_probe", dropped=True, key=None, base=None))
            S.append(dict(first_plan, repeat_of=0))                                       # the first plan's call again: compiled anew, same bytes

    # ---- 6. the ragged base cache: 66 bases, then the first one again (rebuilt) ----------------------------------------------------------
    rag = {n: _proofs("dleq", n, rng, ragged=True) for n in range(2, 68)}
    first = None
    for n in range(2, 68):
        s = verify_step("verify_compact", rag[n], {n - 1} if n % 2 else set(), rng)
        first = first or s
        S.append(s)
    S.append(dict(first, rebuilds_base=True))

    # ---- 7. ZKP_OPT_WS_LIMIT_BYTES below a call's need -----------------------------------------------------------------------------------
    cmz_huge = _proofs("cmz", 1024, rng)
    S.append(option_step("WS_LIMIT_BYTES", 1 << 20))
    S.append(dict(prove_step(cmz_huge), oom=True))
    S.append(prove_step(dleq[11]))
    S.append(option_step("WS_LIMIT_BYTES", 0))
    S.append(prove_step(cmz_huge))
    S.append(verify_step("verify_compact", dleq[6], {2}, rng))
    _CACHE["script"] = S
    return S


class Oom(Exception):
    pass


def run_step(eng, s):
    """one step on `eng` (an Engine of either build; None = the toolbox's host backend) -> what the call returned, in the form of s["expect"]
    (None for steps without a result; Oom for a call the workspace limit refused).  GPU-only steps are the GPU test's."""
    from zkp_amd import toolbox as T
    kind = s["kind"]
    if kind == "option":
        if eng is None:
            return None
        try:
            eng.set_option(s["option"], s["value"])
        except Exception:
            if not s["refused"]:
                raise
            return None
        assert not s["refused"], "option %s = %d should have been refused" % (s["name"], s["value"])
        return None
    if kind == "register":
        if eng is not None:
            eng.prepare_fixed_points(s["encodings"])
        return None
    if kind == "msm_many":
        if eng is None:
            return C.msm_many(s["off"], s["sc"], s["pidx"], s["points"], s["flags"])
        return eng.msm_many(s["off"], s["sc"], s["pidx"], s["points"], s["flags"])
    p = s["p"]
    tst = _statements()[p["which"]][2]
    ts = p["ts0"].copy()
    host = T.HostEngine()
    fst = fused_statement(p["which"]) if eng is not None else None
    if kind == "job":
        if eng is None:                                                    # the host backend has no jobs: the waited job is a plain verification there
            return T.verify_compact_batch(host, tst, ts, p["inst"], p["common"], p["chal"], s["responses"]) if s["mode"] == "wait" else None
        import ctypes
        lib, n = eng._lib, p["n"]
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        inst, common, chal, resp = (np.ascontiguousarray(a, dtype=np.uint8) for a in (p["inst"], p["common"], p["chal"], s["responses"]))
        results = np.zeros(n, np.uint8)                                    # what a careless caller hands over
        rc = lib.zkp_fused_verify_compact_submit(eng._h, ctypes.cast(ctypes.byref(fst.c), ctypes.c_void_p), n, 0, ptr(ts), ptr(inst), n, ptr(common), ptr(chal),
                                                 ptr(resp), None, ptr(results))
        assert rc == 0, lib.zkp_last_error()
        assert results.all() and lib.zkp_ctx_job_pending(eng._h) == 1      # rejected until the job's own copy out says otherwise
        rc = lib.zkp_ctx_job_wait(eng._h) if s["mode"] == "wait" else lib.zkp_ctx_job_discard(eng._h)
        assert rc == 0 and lib.zkp_ctx_job_pending(eng._h) == 0, lib.zkp_last_error()
        return results
    if kind == "prove":
        if eng is None:
            return tuple(T.prove_batch(host, tst, ts, p["secrets"], p["inst"], p["common"], p["entropy"]))
        try:
            got = eng.fused_prove_ragged(fst, ts, p["secrets"], p["inst"], p["common"], p["entropy"])
        except Exception as e:
            if s.get("oom") and "code -4:" in str(e):                  # ZKP_ERR_OOM
                return Oom
            raise
        assert got[3] == 0
        return got[:3]
    if kind == "verify_compact":
        if eng is None:
            return T.verify_compact_batch(host, tst, ts, p["inst"], p["common"], p["chal"], s["responses"])
        return eng.fused_verify_compact_ragged(fst, ts, p["inst"], p["common"], p["chal"], s["responses"])
    if kind == "verify_each":
        if eng is None:
            return T.verify_batchable_each(host, tst, ts, p["inst"], p["common"], p["coms"], s["responses"], s["w"])
        return eng.fused_verify_batchable_ragged(fst, ts, p["inst"], p["common"], p["coms"], s["responses"], s["w"])
    if kind == "batch":
        if eng is None:
            return T.batch_verify_many(host, tst, s["K"], ts, p["inst"], p["common"], p["coms"], s["responses"], s["w"])
        return eng.fused_batch_verify_many_ragged(fst, s["K"], ts, p["inst"], p["common"], p["coms"], s["responses"], s["w"])
    raise ValueError(kind)


def check(s, got):
    """got == s["expect"], byte for byte"""
    exp = s["expect"]
    if isinstance(exp, tuple):
        assert len(got) == len(exp)
        for a, e in zip(got, exp):
            assert np.array_equal(np.asarray(a), np.asarray(e)), s["kind"]
    else:
        assert np.array_equal(np.asarray(got), np.asarray(exp)), (s["kind"], np.asarray(got).tolist()[:16], np.asarray(exp).tolist()[:16])

"""Ragged batches on the device: transcripts at different STROBE positions (signatures over messages of different lengths, the reference's
tests/sig_and_vrf_example.rs) run the fused flows through the _ragged entry points and k_transcript_run_ragged.  Every result, verdict and
transcript left behind must equal the host-transcript route of the same toolbox call byte for byte."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import random

from oracle import cbind as C
from oracle import model as M
from zkp_amd import toolbox as T
from zkp_amd.engine import FusedStatement
from tests.statement_shapes import SHAPES, _materialise, _shape_case
from tests.test_gpu_toolbox import BASEPOINT, _cmz_batch

pytestmark = pytest.mark.gpu
NEVER = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()
    T.set_fused_min_batch(32)


@pytest.fixture(autouse=True)
def _default_routing():
    T.set_fused_min_batch(32)
    yield
    T.set_fused_min_batch(32)


def _rs(rng, k):
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def _mul(scalars, bases, idx):
    n = len(scalars)
    out, st = C.msm_many(np.arange(n + 1, dtype=np.uint32), scalars, np.asarray(idx, np.uint32), bases, 0)
    assert not st.any()
    return out


def _dleq(n, seed):
    rng = np.random.default_rng(seed)
    base = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32)
    x = _rs(rng, n)
    H = _mul(_rs(rng, n), base, np.zeros(n))
    A = _mul(x, base, np.zeros(n))
    B = _mul(x, H, np.arange(n))
    return T.dleq_module().statement, x.reshape(n, 1, 32), np.ascontiguousarray(np.stack([A, B, H])), base.copy()


def _sig(n, seed):
    """sig_proof (sig_and_vrf_example.rs:24): A = x * B, B the basepoint"""
    rng = np.random.default_rng(seed)
    base = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32)
    x = _rs(rng, n)
    A = _mul(x, base, np.zeros(n))
    st = T.define_proof("sig", b"Sig", ["x"], ["A"], ["B"], [("A", [("x", "B")])]).statement
    return st, x.reshape(n, 1, 32), np.ascontiguousarray(A[None]), base.copy()


def _cmz(n, seed):
    mod, secrets, inst, common = _cmz_batch(n, seed)
    return mod.statement, secrets, inst, common


def _shape(name):
    def make(n, seed):
        shape, secrets_int, dlog = _shape_case(name, n, np.random.default_rng(seed))
        secrets, inst, common = _materialise(shape, n, secrets_int, dlog)
        return shape.build()[0], secrets, inst, common
    return make


def _ragged_msgs(n, rng, label=b"SigTest", lens=None):
    """n transcripts after append_message(b"msg", m) with lengths that cover every STROBE position -> (states, messages)"""
    if lens is None:
        lens = [(j * 37) % 166 + 166 * int(rng.integers(0, 3)) for j in range(n)]
    msgs = [rng.bytes(k) for k in lens]
    return T.append_messages(label, b"msg", msgs), msgs


def _ragged(n, rng, label=b"SigTest", lens=None):
    return _ragged_msgs(n, rng, label, lens)[0]


def _model_proof_check(st, label, msg, j, secrets, inst, common, entropy, chal, resp, coms):
    """proof j against the oracle model's prover (prover.rs:76-112) on Transcript::new(label) + append_message(b"msg", msg)"""
    t = M.Transcript(label)
    t.append_message(b"msg", msg)
    mp = M.Prover(st.proof_label, t)
    sv = [mp.allocate_scalar(name, int.from_bytes(secrets[j, i].tobytes(), "little")) for i, name in enumerate(st.secrets)]
    pv, ki, kc = [], 0, 0
    for name, is_common in st.points:
        enc = common[kc] if is_common else inst[ki, j]
        kc, ki = kc + is_common, ki + (not is_common)
        pv.append(mp.allocate_point(name, M.ristretto_decode(enc.tobytes()))[0])
    for lhs, lc in st.constraints:
        mp.constrain(pv[lhs], [(sv[s_], pv[p_]) for s_, p_ in lc])
    c, r, k, _ = mp._prove_impl(entropy[j].tobytes())
    assert chal[j].tobytes() == M.sc_to_bytes(c), j
    assert [x.tobytes() for x in resp[j]] == [M.sc_to_bytes(v) for v in r], j
    assert [x.tobytes() for x in coms[j]] == [bytes(x) for x in k], j


def _prove_both(eng, st, ts0, secrets, inst, common, entropy):
    out = {}
    for route, thr in (("dev", 32), ("host", NEVER)):
        T.set_fused_min_batch(thr)
        ts = ts0.copy()
        out[route] = T.prove_batch(eng, st, ts, secrets, inst, common, entropy) + (ts,)
    T.set_fused_min_batch(32)
    for a, b in zip(out["dev"][:3], out["host"][:3]):
        assert (a == b).all()
    assert (out["dev"][3][:, :203] == out["host"][3][:, :203]).all()
    return out["dev"]


def test_ragged_dleq_prove_runs_the_ragged_kernel(eng):
    """the toolbox's defaults send a ragged batch of 300 DLEQ proofs to the device, and the device equals the host route"""
    n = 300
    rng = np.random.default_rng(1)
    st, x, inst, common = _dleq(n, 2)
    ts0 = _ragged(n, rng)
    assert len({bytes(r[200:203]) for r in ts0}) > 100
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    eng.set_profiling(True)
    try:
        ts = ts0.copy()
        got = T.prove_batch(eng, st, ts, x, inst, common, entropy)
        assert "zkp::k_transcript_run_ragged" in eng.last_kernels().get("transcript", [])
    finally:
        eng.set_profiling(False)
    T.set_fused_min_batch(NEVER)
    ts_h = ts0.copy()
    want = T.prove_batch(eng, st, ts_h, x, inst, common, entropy)
    for a, b in zip(got, want):
        assert (a == b).all()
    assert (ts[:, :203] == ts_h[:, :203]).all()


RANDOM_SHAPES = random.Random(2024).sample(SHAPES, 2)      # two statements of tests/statement_shapes.py, chosen once by a fixed seed
MAKERS = {"dleq": _dleq, "sig": _sig, "cmz": _cmz, **{s_: _shape(s_) for s_ in RANDOM_SHAPES}}
CASES = [(k, n) for k in ("dleq", "sig", "cmz") for n in (32, 300, 4096)] + [(s_, n) for s_ in RANDOM_SHAPES for n in (32, 300)]


@pytest.mark.parametrize("kind,n", CASES)
def test_ragged_flows_equal_host_route(eng, kind, n):
    rng = np.random.default_rng(n + len(kind))
    st, secrets, inst, common = MAKERS[kind](n, 7)
    ts0, msgs = _ragged_msgs(n, rng)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    chal, resp, coms, _ = _prove_both(eng, st, ts0, secrets, inst, common, entropy)
    if kind != "cmz":                                   # (the model's prover is pure Python: CMZ's 21 secrets take too long)
        for j in (0, n // 3, n - 1):
            _model_proof_check(st, b"SigTest", msgs[j], j, secrets, inst, common, entropy, chal, resp, coms)
    bad = sorted({1, n // 2, n - 1})
    resp_bad = resp.copy()
    for j in bad:
        resp_bad[j, 0, 0] ^= 1
    # verify_compact: honest accepted, mutants rejected exactly; same transcripts as the host route
    for r, want in ((resp, []), (resp_bad, bad)):
        res = {}
        for route, thr in (("dev", 32), ("host", NEVER)):
            T.set_fused_min_batch(thr)
            ts = ts0.copy()
            res[route] = (T.verify_compact_batch(eng, st, ts, inst, common, chal, r), ts)
        T.set_fused_min_batch(32)
        assert np.flatnonzero(res["dev"][0]).tolist() == want and (res["dev"][0] == res["host"][0]).all()
        assert (res["dev"][1][:, :203] == res["host"][1][:, :203]).all()
    # verify_batchable_each
    w_each = rng.integers(0, 256, size=(n, st.nc, 16), dtype=np.uint8)
    for r, want in ((resp, []), (resp_bad, bad)):
        assert np.flatnonzero(T.verify_batchable_each(eng, st, ts0.copy(), inst, common, coms, r, w_each)).tolist() == want
    # batch_verify, batch_verify_many, batch_verify_locate
    w = rng.integers(0, 256, size=(st.nc, n, 16), dtype=np.uint8)
    ts = ts0.copy()
    T.batch_verify(eng, st, ts, inst, common, coms, resp, w)
    T.set_fused_min_batch(NEVER)
    ts_h = ts0.copy()
    T.batch_verify(eng, st, ts_h, inst, common, coms, resp, w)
    T.set_fused_min_batch(32)
    assert (ts[:, :203] == ts_h[:, :203]).all()
    T.batch_verify(eng, st, ts0.copy(), inst, common, coms, resp)                      # weights drawn on the device
    one = resp.copy()
    one[n // 2, 0, 0] ^= 1
    with pytest.raises(T.VerificationFailure):
        T.batch_verify(eng, st, ts0.copy(), inst, common, coms, one, w)
    ok, where = T.batch_verify_locate(eng, st, ts0.copy(), inst, common, coms, one)
    assert not ok and np.flatnonzero(where).tolist() == [n // 2]
    if n % 2 == 0:
        assert T.batch_verify_many(eng, st, 2, ts0.copy(), inst, common, coms, resp).tolist() == [0, 0]
        assert T.batch_verify_many(eng, st, 2, ts0.copy(), inst, common, coms, one, w).tolist() == [0, 1]      # n // 2 lies in the second batch


def test_ragged_identity_point_rejected_alone(eng):
    n = 300
    rng = np.random.default_rng(5)
    st, x, inst, common = _dleq(n, 6)
    ts0 = _ragged(n, rng)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    chal, resp, coms, _ = _prove_both(eng, st, ts0, x, inst, common, entropy)
    inst_bad = inst.copy()
    inst_bad[0, 17] = 0                                  # A of proof 17 = the identity's encoding: the validating append rejects it
    res = T.verify_compact_batch(eng, st, ts0.copy(), inst_bad, common, chal, resp)
    assert np.flatnonzero(res).tolist() == [17]
    T.set_fused_min_batch(NEVER)
    assert (T.verify_compact_batch(eng, st, ts0.copy(), inst_bad, common, chal, resp) == res).all()
    T.set_fused_min_batch(32)
    w = rng.integers(0, 256, size=(n, st.nc, 16), dtype=np.uint8)
    assert np.flatnonzero(T.verify_batchable_each(eng, st, ts0.copy(), inst_bad, common, coms, resp, w)).tolist() == [17]


def test_one_proof_per_class(eng):
    n = 166
    rng = np.random.default_rng(8)
    st, x, inst, common = _dleq(n, 9)
    ts0 = _ragged(n, rng, lens=list(range(166)))
    assert len({bytes(r[200:203]) for r in ts0}) == 166
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    chal, resp, coms, _ = _prove_both(eng, st, ts0, x, inst, common, entropy)
    assert not T.verify_compact_batch(eng, st, ts0.copy(), inst, common, chal, resp).any()
    T.batch_verify(eng, st, ts0.copy(), inst, common, coms, resp)


def test_aligned_batch_with_one_straggler(eng):
    n = 4096
    rng = np.random.default_rng(10)
    st, x, inst, common = _dleq(n, 11)
    ts0 = _ragged(n, rng, lens=[40] * (n - 1) + [41])
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    chal, resp, coms, _ = _prove_both(eng, st, ts0, x, inst, common, entropy)
    T.batch_verify(eng, st, ts0.copy(), inst, common, coms, resp)
    one = resp.copy()
    one[n - 1, 0, 0] ^= 1
    ok, where = T.batch_verify_locate(eng, st, ts0.copy(), inst, common, coms, one)
    assert not ok and np.flatnonzero(where).tolist() == [n - 1]


def test_very_wide_ragged_dleq(eng):
    """70,000 proofs: above kVeryWideCallProofs (65,536), where aligned calls switch transcript schedules; a ragged call keeps its kernel"""
    base_n, reps = 4096, 18
    n = 70000
    st, x, inst, common = _dleq(base_n, 12)
    x = np.tile(x, (reps, 1, 1))[:n]
    inst = np.ascontiguousarray(np.tile(inst, (1, reps, 1))[:, :n])
    rng = np.random.default_rng(13)
    ts0 = _ragged(n, rng)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    chal, resp, coms, _ = _prove_both(eng, st, ts0, x, inst, common, entropy)
    T.batch_verify(eng, st, ts0.copy(), inst, common, coms, resp)


def test_seeded_ragged_prove(eng):
    n = 300
    rng = np.random.default_rng(14)
    st, x, inst, common = _dleq(n, 15)
    ts0 = _ragged(n, rng)
    c1, r1, k1 = T.prove_batch(eng, st, ts0.copy(), x, inst, common)
    c2, r2, k2 = T.prove_batch(eng, st, ts0.copy(), x, inst, common)
    assert not (c1 == c2).all(axis=1).any() and not (k1 == k2).all(axis=(1, 2)).any()
    assert not T.verify_compact_batch(eng, st, ts0.copy(), inst, common, c1, r1).any()
    T.batch_verify(eng, st, ts0.copy(), inst, common, k2, r2)


def test_hash_to_group_on_ragged_transcripts(eng):
    n = 300
    rng = np.random.default_rng(16)
    ts0 = _ragged(n, rng, label=b"VRF")
    eng.set_profiling(True)
    try:
        ts = ts0.copy()
        out = T.hash_to_group(eng, ts)
        assert "zkp::k_transcript_run_ragged" in eng.last_kernels().get("transcript", [])
    finally:
        eng.set_profiling(False)
    ts_h = ts0.copy()
    want = T.hash_to_group(None, ts_h)                   # the host backend: host Merlin and the map on the host cores
    assert (out == want).all() and (ts == ts_h).all()
    ts_e = ts0.copy()
    assert (eng.fused_hash_to_group_ragged(ts_e) == want).all() and (ts_e == ts_h).all()


DLEQ_FST = lambda: FusedStatement(b"DLEQ proof", [b"x"], [(b"A", False), (b"B", False), (b"H", False), (b"G", True)], [(0, [(0, 3)]), (1, [(0, 2)])])


def test_program_cache_compiles_each_class_once():
    """Class programs and the position-free base plan are compiled once per context: a second call with the same classes in another order
    (another proof 0) compiles nothing, and ragged calls never add to or flush the aligned plan cache"""
    from zkp_amd.engine import Engine
    n = 300
    rng = np.random.default_rng(17)
    st, x, inst, common = _dleq(n, 18)
    fst = DLEQ_FST()
    ts0 = _ragged(n, rng)
    n_cls = len({bytes(r[200:203]) for r in ts0})
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    perm = np.random.default_rng(3).permutation(n)
    assert bytes(ts0[perm[0], 200:203]) != bytes(ts0[0, 200:203])
    eh = Engine(0, test_hooks=True)
    try:
        aligned = _ragged(n, rng, lens=[9] * n)
        eh.fused_prove_ragged(fst, aligned, x, inst, common, entropy)                    # one aligned plan
        first = eh.fused_prove_ragged(fst, ts0.copy(), x, inst, common, entropy)
        s1 = eh.last_schedule()
        second = eh.fused_prove_ragged(fst, np.ascontiguousarray(ts0[perm]), x[perm], np.ascontiguousarray(inst[:, perm]), common, entropy[perm])
        s2 = eh.last_schedule()
        # many calls whose proof 0 stands at every position in turn: still one aligned plan, no base plan or class program built
        for k in range(0, n, 3):
            order = np.roll(np.arange(n), -k)
            eh.fused_prove_ragged(fst, np.ascontiguousarray(ts0[order]), x[order], np.ascontiguousarray(inst[:, order]), common, entropy[order])
            s3 = eh.last_schedule()
            assert s3["ragged_compiled"] == 0 and s3["ragged_base"] == 0 and s3["fused_plans"] == 1, (k, s3)
        # the other flows build their own base plans once
        eh.fused_verify_compact_ragged(fst, ts0.copy(), inst, common, first[0], first[1])
        s4 = eh.last_schedule()
        eh.fused_verify_compact_ragged(fst, np.ascontiguousarray(ts0[perm]), np.ascontiguousarray(inst[:, perm]), common, first[0][perm], first[1][perm])
        s5 = eh.last_schedule()
    finally:
        eh.close()
    assert s1["ragged_classes"] == n_cls and s1["ragged_compiled"] == n_cls and s1["ragged_base"] == 1 and s1["fused_plans"] == 1
    assert s2["ragged_classes"] == n_cls and s2["ragged_compiled"] == 0 and s2["ragged_base"] == 0 and s2["fused_plans"] == 1
    assert s1["tr_steps"] == 0 and s1.get("fuse_tt", 0) == 0
    assert s4["ragged_base"] == 1 and s4["ragged_compiled"] == n_cls and s5["ragged_base"] == 0 and s5["ragged_compiled"] == 0
    assert s5["fused_plans"] == 1
    for a, b in zip(first[:3], second[:3]):
        assert (a[perm] == b).all()
    want = T.prove_batch(T.HostEngine(), st, ts0.copy(), x, inst, common, entropy)       # the host backend
    for a, b in zip(first[:3], want):
        assert (a == b).all()


def test_raw_entries_refuse_ragged_and_ragged_entries_take_aligned(eng):
    n = 64
    rng = np.random.default_rng(19)
    st, x, inst, common = _dleq(n, 20)
    fst = DLEQ_FST()
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    aligned = _ragged(n, rng, lens=[9] * n)
    got = eng.fused_prove_ragged(fst, aligned.copy(), x, inst, common, entropy)
    ts = aligned.copy()
    want = T.prove_batch(eng, st, ts, x, inst, common, entropy)                        # aligned: zkp_fused_prove
    for a, b in zip(got[:3], want):
        assert (a == b).all()
    assert got[3] == 0
    ragged = _ragged(n, rng)
    lib = eng._lib
    res = np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.zkp_fused_verify_compact(eng._h, ctypes.byref(fst.c), ctypes.c_uint32(n), p(ragged), p(inst), p(common), p(want[0]), p(want[1]), p(res))
    assert rc < 0 and b"STROBE" in lib.zkp_last_error()
    out = np.zeros((n, 32), np.uint8)
    assert lib.zkp_fused_hash_to_group(eng._h, n, p(ragged), b"output", p(out)) < 0
    with pytest.raises(Exception):
        eng.fused_prove_ragged(fst, ragged.copy(), x, inst, common, entropy, seed=bytes(40))   # entropy and seed: exactly one


def test_sig_batch_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sig_batch.py"), "4096"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

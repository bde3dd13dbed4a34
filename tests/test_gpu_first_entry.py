"""Chains of additions that start at their first entry, the two forms of the Pippenger bucket merge, and the carry window of reduced scalars.

* zkp_msm_optional with scalars chosen so that buckets hold 0, 1, 2, L - 1, L, L + 1, 2 L - 1 and 2 L + 1 entries (L = 16, the part length)
  and one bucket is huge (more than 128 parts of 4 L entries: the block-wide sum): a quad per bucket, a lane per bucket and the default
  choice give the oracle's bytes.
* zkp_batch_verify_many with 212 and 213 batches, whose 2,470 buckets each put the call on either side of the 2^19 buckets from which
  the merge takes a lane per bucket (zkp_debug_last_schedule: pip_merge, pip_buckets); both forms forced on both sides; the verdicts are
  the oracle's.
* the fused CMZ prover on the throughput and the latency schedule skips the carry window (no_carry = 1): witnesses 0, 1, l - 1 and
  non-canonical strings among ordinary ones, byte for byte against oracle/c.
* a raw constant-time zkp_msm_many call with multipliers >= 2^255 keeps the window (no_carry = 0) and matches the oracle.
"""
import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from zkp_amd import engine as EN
from zkp_amd import toolbox as T
from tests import degenerate_cases as D
from tests.test_gpu_fused import _dleq_batch

pytestmark = pytest.mark.gpu
BASE = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8).reshape(1, 32)
PART = 16                                   # pip_part of calls below 2^18 terms
MERGE_LANE_MIN_BUCKETS = 1 << 19            # pip_run: the lane form from this many buckets (batches x windows x buckets per window) on


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0, test_hooks=True)
    yield e
    e.close()
    T.set_fused_min_batch(32)


def _sc(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8)


def _points(k, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    pts, _ = C.msm_many(np.arange(k + 1, dtype=np.uint32), s, np.zeros(k, np.uint32), BASE, 0)
    return pts


def test_msm_optional_bucket_sizes_on_both_merge_forms(eng):
    rng = np.random.default_rng(16)
    L = PART
    # small positive scalars d < 2^10 have the single signed digit d in window 0 (c = 11): bucket d of window 0 gets one entry per copy;
    # l - d is folded to -d: the same bucket, negated entry
    counts = {3: 1, 4: 2, 5: L - 1, 6: L, 7: L + 1, 8: 2 * L - 1, 9: 2 * L + 1, 10: 4 * L, 11: 4 * L + 1, 12: 128 * 4 * L + 77}      # (bucket 2: no entry)
    scal = []
    for d, k in counts.items():
        scal += [_sc(d if i % 3 else M.L - d) for i in range(k)]
    scal += [_sc(int.from_bytes(rng.bytes(32), "little") % M.L) for _ in range(700)]                # every window populated
    scal = np.stack(scal)
    rng.shuffle(scal, axis=0)
    n = len(scal)
    assert 8192 <= n < (1 << 18)
    pts24 = _points(24, 17)
    pts = pts24[rng.integers(0, 24, size=n)]
    want = C.msm_optional(scal, pts)
    assert want is not None
    try:
        for mode, form in ((0, 0), (1, 0), (2, 1)):
            eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, mode)
            got = eng.msm_optional(scal, pts)
            sched = eng.last_schedule()
            assert sched["opt_pip"] == 1 and sched["pip_c"] == 11 and sched["pip_part"] == L and sched["pip_merge"] == form, (mode, sched)
            assert got == want, "merge mode %d" % mode
        # an undecodable point is still reported, whatever the form
        bad = pts.copy()
        bad[n // 2] = np.frombuffer(bytes([1] + [0] * 31), np.uint8)
        for mode in (1, 2):
            eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, mode)
            assert eng.msm_optional(scal, bad) is None
    finally:
        eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, 0)


@pytest.mark.parametrize("K", [212, 213])
def test_batch_verify_many_on_both_sides_of_the_merge_rule(eng, K):
    """DLEQ, two proofs per batch: 1 + 5 * 2 terms per batch MSM, c = 7, 38 windows x 65 buckets = 2,470 buckets per batch"""
    n_each = 2
    n = K * n_each
    per_batch = 38 * 65
    assert 212 * per_batch < MERGE_LANE_MIN_BUCKETS <= 213 * per_batch
    mod, x, A, B, H = _dleq_batch(n, 30 + K)
    st = mod.statement
    fst = EN.FusedStatement(st.proof_label, st.secrets, st.points, st.constraints)
    inst = np.ascontiguousarray(np.stack([A, B, H]))
    common = BASE.copy()
    label = b"merge-rule"
    entropy = np.random.default_rng(K).integers(0, 256, size=(n, 32), dtype=np.uint8)
    # (the toolbox library drives contexts of the SHIPPED library only: the proofs are made on a plain engine, the test-hook engine verifies them)
    plain = EN.Engine(0)
    T.set_fused_min_batch(0)
    try:
        ts = np.stack([T.Transcript(label).state] * n)
        chal, resp, coms = T.prove_batch(plain, st, ts, x, inst, common, entropy)
    finally:
        plain.close()
        T.set_fused_min_batch(32)
    try:
        w = np.random.default_rng(K + 1).integers(0, 256, size=(st.nc, n, 16), dtype=np.uint8)
        bad = resp.copy()
        tampered = [0, 97, K - 1]
        for b in tampered:
            bad[b * n_each + 1, 0, 3] ^= 0x10
        expect = np.zeros(K, np.int32)
        expect[tampered] = 1
        for mode in (0, 1, 2):
            eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, mode)
            ts = np.stack([T.Transcript(label).state] * n)
            v = eng.fused_batch_verify_many(fst, K, ts, inst, common, coms, resp, w)
            sched = eng.last_schedule()
            assert sched["pip_c"] == 7 and sched["pip_buckets"] == K * per_batch, sched
            form = {0: int(K * per_batch >= MERGE_LANE_MIN_BUCKETS), 1: 0, 2: 1}[mode]
            assert sched["pip_merge"] == form, (mode, sched)
            assert not v.any(), (mode, np.nonzero(v)[0][:8])
            ts = np.stack([T.Transcript(label).state] * n)
            v = eng.fused_batch_verify_many(fst, K, ts, inst, common, coms, bad, w)
            assert (v == expect).all(), (mode, np.nonzero(v != expect)[0][:8])
    finally:
        eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, 0)
    cst = C.Statement.from_model(M.dleq_statement())
    for b in (0, 1, 97, 150, K - 1):
        sl = slice(b * n_each, (b + 1) * n_each)
        rc = C.batch_verify(cst, label, n_each, np.ascontiguousarray(inst[:, sl]), common, coms[sl], bad[sl], np.ascontiguousarray(w[:, sl]))
        assert rc == expect[b], b


@pytest.mark.parametrize("schedule", ["throughput", "latency"])
def test_fused_cmz_prover_skips_the_carry_window(schedule):
    """degenerate witnesses (0, 1, l - 1, the sign-fold boundary, non-canonical strings: tests/degenerate_cases.py) among ordinary ones; the walks'
    scalars are the blindings, reduced mod l whatever the witnesses are"""
    import torch
    assert torch.cuda.is_available(), "torch cannot see the GPU in this process"
    n = 300
    b = D.build_batch("cmz10", n, D.dense_plan("cmz10", n), n)
    _, cst = b.shape.build()
    rng = np.random.default_rng(n)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    e = EN.Engine(0, test_hooks=True)
    try:
        e.set_option(EN.ZKP_OPT_DEV_OVERLAP, 2 if schedule == "latency" else 0)
        import bench
        fst = EN.FusedStatement(b"CMZ cred show n=10", *bench.cmz_statement())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
        t0 = T.Transcript(b"no-carry").state
        pos = int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16
        e.prepare_fixed_points(b.common)
        d_tbl = dev(np.concatenate([b.common, b.inst.reshape(-1, 32)]))
        d_ts, d_sec, d_ent = dev(np.stack([t0] * n)), dev(b.secrets), dev(entropy)
        d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, 21, 32), z(n, 11, 32), z(11 * n)
        torch.cuda.synchronize()
        e.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                          d_coms.data_ptr(), d_st.data_ptr())
        e.synchronize()
        sched = e.last_schedule()
        assert sched.get("terms_split") == 1 and sched.get("no_carry") == 1, sched
        assert not d_st.cpu().numpy().any()
        chal, resp, coms = d_chal.cpu().numpy(), d_resp.cpu().numpy(), d_coms.cpu().numpy()
    finally:
        e.close()
    assert b.degenerate
    for j in range(n):
        ec, er, ek, _ = C.prove(cst, b"no-carry", b.secrets[j], D.points_of(b, j), entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), "proof %d differs from the oracle's" % j


def test_raw_constant_time_call_keeps_the_carry_window(eng):
    """zkp_msm_many takes any 256-bit multiplier: s + 0x88...8 carries out of bit 255 for s >= 2^255 - 0x88...8, and the 65th addition stays"""
    rng = np.random.default_rng(255)
    n_pts, n_msm, per = 40, 128, 11
    pts = _points(n_pts, 256)
    n_terms = n_msm * per
    assert n_terms >= 1024
    sc = rng.integers(0, 256, size=(n_terms, 32), dtype=np.uint8)
    sc[::2, 31] |= 0x80                                            # >= 2^255
    sc[1::4, 31] |= 0xf0                                           # carries out of bit 255 in the radix-16 recoding
    sc[5] = 0xff
    sc[6] = _sc((1 << 256) - 1 - int("88" * 32, 16))              # the largest multiplier without the carry
    sc[7] = _sc((1 << 256) - int("88" * 32, 16))                  # the smallest with it
    off = np.arange(0, n_terms + 1, per, dtype=np.uint32)
    # per MSM: one point used by many terms of the call (comb tables, grouped walk) and points used once or twice
    pidx = rng.integers(0, n_pts, size=n_terms).astype(np.uint32)
    pidx[::per] = 0
    want, west = C.msm_many(off, sc, pidx, pts, 1)
    for grouped in (2**64 - 1, 1):
        eng.set_option(EN.ZKP_OPT_GROUPED_COMB, grouped)
        try:
            got, st = eng.msm_many(off, sc, pidx, pts, EN.ZKP_CT)
        finally:
            eng.set_option(EN.ZKP_OPT_GROUPED_COMB, 2**64 - 1)
        sched = eng.last_schedule()
        assert sched.get("terms_split") == 1 and sched.get("no_carry") == 0, sched
        assert (st == west).all() and (got == want).all(), grouped

"""Degenerate witnesses and coinciding points (tests/degenerate_cases.py) on the device: the toolbox routes (host transcripts with device
MSMs, fused, ragged-fused), the _dev entry points under every schedule and term-path option, CMZ on both sides of the size thresholds
that change the term path, and the seeded synchronous calls.  Every expected byte and verdict comes from oracle/c (and oracle/model.py
for samples); tests/test_host_degenerate.py runs the same table on the host backend without a GPU.

Sizes: whole-family batches at 200 proofs; mixed batches (degenerate proofs at 0, 31, 32, 63, 64, 255, 256, n - 1 among ordinary ones) at 200
and 1,024.  The oracle recomputes EVERY proof and verdict of every batch on one core, which is what this module's time goes to: with mixed
batches of 4,096 the module took 198 s where tests/test_gpu_fused.py takes 7 s, with 1,024 it takes 115 s.  Families were not cut.  At
1,024 proofs the CMZ batch MSM (24,588 terms) is still above the Pippenger rows of tests/size_thresholds.py (4,096 / 8,192 terms), and
the term-path rows 6 and 8 have their own cases below."""
import ctypes

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from zkp_amd import engine as EN
from zkp_amd import toolbox as T
from tests import degenerate_cases as D
from tests import statement_shapes as SH
from tests.statement_shapes import NEVER
from tests.test_host_degenerate import _names, check_model_sample

pytestmark = pytest.mark.gpu
N_WHOLE, N_MIXED = 200, (200, 1024)
WHOLE = [(s, f) for s in D.STATEMENTS for f in D.families_of(s)]
MIXED = [(s, n, b) for s in D.STATEMENTS for n in N_MIXED for b in range(len(D.mixed_plans(s, n)))]
ROUTES = (("host", NEVER), ("fused", 0))


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0)
    yield e
    e.close()
    T.set_fused_min_batch(32)


_torch = SH._torch


def _expect(b, seed, **kw):
    return SH.oracle_expectation(b.shape, b.n, b.secrets, b.inst, b.common, seed, b.ordinary, same_entropy=b.same_entropy, **kw)


# ---- the toolbox routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stname,fam", WHOLE, ids=["%s-%s" % c for c in WHOLE])
def test_whole_family_batches_on_both_routes_vs_oracle(eng, stname, fam):
    n = N_WHOLE
    b = D.whole_batch(stname, fam, n, D.seed_of(stname, fam, n))
    E = _expect(b, n)
    eng.prepare_fixed_points(b.common[:64])
    SH._check_flows_vs_oracle(eng, b.shape, n, b.secrets, b.inst, b.common, E, routes=ROUTES, names=_names(b))


def _ragged_routes(eng, b, E, rng):
    """The same batch on transcripts that stand at different STROBE positions (a message of another length appended to each): the host
    route and the ragged-fused route must give the same bytes and leave the same states; a sample equals oracle/model.py; and each proof
    gets the verdict the oracle gave the aligned proof of the same inputs (an identity point is refused whatever the transcript holds)."""
    n, st = b.n, b.shape.build()[0]
    msgs = [rng.bytes((j * 37) % 166 + 166 * int(rng.integers(0, 3))) for j in range(n)]
    t0 = T.append_messages(E.tl, b"msg", msgs)
    out = {}
    for route, thr in ROUTES:
        T.set_fused_min_batch(thr)
        try:
            ts = t0.copy()
            chal, resp, coms = T.prove_batch(eng, st, ts, b.secrets, b.inst, b.common, E.entropy)
            ts2 = t0.copy()
            res = T.verify_compact_batch(eng, st, ts2, b.inst, b.common, chal, resp)
            each = T.verify_batchable_each(eng, st, t0.copy(), b.inst, b.common, coms, resp, E.w_each)
            acc = E.vb == 0
            sub = lambda a, axis=0: np.ascontiguousarray(np.compress(acc, a, axis=axis))
            try:
                T.batch_verify(eng, st, sub(t0), sub(b.inst, 1), b.common, sub(coms), sub(resp), sub(E.w, 1))
                rc = 0
            except T.VerificationFailure:
                rc = 1
        finally:
            T.set_fused_min_batch(32)
        assert (res == E.vc).all() and (each == E.vb).all(), (route, np.nonzero(res != E.vc)[0][:8], np.nonzero(each != E.vb)[0][:8])
        assert rc == 0, "%s route: the proofs the oracle accepts one by one fail as a batch" % route
        out[route] = (chal, resp, coms, ts[:, :203], ts2[E.vc == 0][:, :203])
    for x, y in zip(out["host"], out["fused"]):
        assert (x == y).all(), "the host route and the ragged-fused route leave different bytes"
    chal, resp, coms = out["fused"][:3]
    j = sorted(b.degenerate)[int(rng.integers(0, len(b.degenerate)))]
    t = M.Transcript(E.tl)
    t.append_message(b"msg", msgs[j])
    mc, mr, mk = D.model_prove(b.shape, t, b.secrets[j], D.points_of(b, j), E.entropy[j].tobytes())
    assert (mc == chal[j]).all() and (mr == resp[j]).all() and (mk == coms[j]).all(), "ragged proof %d (%s) differs from the model's" % (j, _names(b)[j])
    t = M.Transcript(E.tl)
    t.append_message(b"msg", msgs[j])
    assert D.model_verify_compact(b.shape, t, D.points_of(b, j), chal[j], resp[j]) == E.vc[j]


@pytest.mark.parametrize("stname,n,k", MIXED, ids=["%s-%d-batch%d" % c for c in MIXED])
def test_mixed_batches_on_all_routes_vs_oracle(eng, stname, n, k):
    """degenerate proofs at lane, wavefront and ragged-block edges among ordinary ones: each changes its own verdict only"""
    plan = D.mixed_plans(stname, n)[k]
    b = D.build_batch(stname, n, plan, D.seed_of(stname, n, k))
    E = _expect(b, n + k)
    ordinary = [j for j in range(n) if j not in plan]
    assert not E.vc[ordinary].any() and not E.vb[ordinary].any()
    eng.prepare_fixed_points(b.common[:64])
    SH._check_flows_vs_oracle(eng, b.shape, n, b.secrets, b.inst, b.common, E, routes=ROUTES, names=_names(b))
    check_model_sample(b, E, sorted(plan)[k % len(plan)])
    _ragged_routes(eng, b, E, np.random.default_rng(n + k))


@pytest.mark.parametrize("whole", [True, False])
def test_identity_commitments_through_the_batched_encoder(whole):
    """A = x P + x (-P): the honest commitment is the identity, which the batched encoder (k_encode_prepare / _finish: one shared inversion
    per 256 outputs) takes out of the product through its zflag branch.  Calls of this size encode per lane by default, so the batched
    encoder is switched on from the first output (ZKP_OPT_BATCH_ENCODE_MIN = 0) -- in a batch where every commitment of A is the identity,
    and in one where identity commitments sit at the placement indices among ordinary ones and share their inversion."""
    n = N_WHOLE
    b = D.whole_batch("cancelling_pair", "neg_cancel", n, 4) if whole else D.build_batch("cancelling_pair", n, {j: "neg_cancel" for j in D.placement(n)}, 5)
    E = _expect(b, n)
    assert (E.coms[sorted(b.degenerate), 0] == 0).all() and E.vc[sorted(b.degenerate)].all()
    e = EN.Engine(0)
    try:
        e.set_option(EN.ZKP_OPT_BATCH_ENCODE_MIN, 0)
        SH._check_flows_vs_oracle(e, b.shape, n, b.secrets, b.inst, b.common, E, routes=ROUTES, names=_names(b))
    finally:
        e.close()


def test_identity_points_are_refused_at_allocation_on_the_device_too(eng):
    with pytest.raises(T.VerificationFailure):
        T.Verifier(b"DLEQProof", T.Transcript(b"degenerate"), eng).allocate_point(b"A", bytes(32))
    with pytest.raises(T.VerificationFailure):
        T.BatchVerifier(b"DLEQProof", 1, [T.Transcript(b"degenerate")], eng).allocate_instance_point(b"A", [bytes(32)])


# ---- the _dev entry points (CMZ: paired terms, riders' tables, comb tables per point slot) ---------------------------------------------------------
# every schedule / term-path configuration tests/test_gpu_device_entry.py parametrises, by the option names of zkp_amd/engine.py
O = EN
DEV_CONFIGS = {
    "default": {},
    "latency": {O.ZKP_OPT_DEV_OVERLAP: 2},
    "interp": {O.ZKP_OPT_TRANSCRIPT_STEPS: 0},
    "one_lane": {O.ZKP_OPT_TRANSCRIPT_LANES: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0},
    "one_lane+interp": {O.ZKP_OPT_TRANSCRIPT_LANES: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0, O.ZKP_OPT_TRANSCRIPT_STEPS: 0},
    "fuse": {O.ZKP_OPT_FUSE_TABLES_TRANSCRIPT: 1},
    "fuse+interp": {O.ZKP_OPT_FUSE_TABLES_TRANSCRIPT: 1, O.ZKP_OPT_TRANSCRIPT_STEPS: 0},
    "fuse+one_lane": {O.ZKP_OPT_FUSE_TABLES_TRANSCRIPT: 1, O.ZKP_OPT_TRANSCRIPT_LANES: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0},
    "single_use_tables": {O.ZKP_OPT_CT_SINGLE_USE_TABLES: 1},
    "single_use_ladder": {O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0},
    "grouped": {O.ZKP_OPT_GROUPED_COMB: 1},
    "grouped+single_use_tables": {O.ZKP_OPT_GROUPED_COMB: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 1},
    "comb_split": {O.ZKP_OPT_COMB_SPLIT: 1},
    "comb_split+latency": {O.ZKP_OPT_COMB_SPLIT: 1, O.ZKP_OPT_DEV_OVERLAP: 2},
    "ladder_interleave": {O.ZKP_OPT_LADDER_INTERLEAVE: 1, O.ZKP_OPT_GROUPED_COMB: 1},
    "pairs+riders_tables": {O.ZKP_OPT_JOINT_LADDER: 1},                      # the throughput schedule of the _dev calls builds the riders' tables
    "pairs+riders_tables+latency": {O.ZKP_OPT_JOINT_LADDER: 1, O.ZKP_OPT_DEV_OVERLAP: 2},
    "pairs_without_tables": {O.ZKP_OPT_JOINT_LADDER: 2},
    "separate_terms": {O.ZKP_OPT_JOINT_LADDER: 0},
}
N_DEV = 300
_DEV_CACHE = {}


def _cmz_fst():
    import bench
    return EN.FusedStatement(b"CMZ cred show n=10", *bench.cmz_statement())


def _dev_case(batch_family):
    """one CMZ batch with every proof-level family in it (or one batch-level family), its oracle expectation, and the oracle's verdict for
    the batch of the proofs it accepts one by one"""
    if batch_family not in _DEV_CACHE:
        n = N_DEV
        if batch_family is None:
            b = D.build_batch("cmz10", n, D.dense_plan("cmz10", n), 77)
            assert {f for f, _ in b.degenerate.values()} == set(D.families_of("cmz10", "proof"))
        else:
            b = D.whole_batch("cmz10", batch_family, n, 78)
        E = _expect(b, 79, many=False)
        acc = E.vb == 0
        assert acc.any()
        if batch_family is None:
            assert not acc.all(), "the dense batch holds refused families (zero_secrets, w:0, ...)"
        _, cst = b.shape.build()
        sub = lambda a, axis=0: np.ascontiguousarray(np.compress(acc, a, axis=axis))
        E.sub = (int(acc.sum()), sub(b.inst, 1), sub(E.coms), sub(E.resp), sub(E.w, 1))
        E.rc_sub = int(C.batch_verify(cst, E.tl, E.sub[0], E.sub[1], b.common, E.sub[2], E.sub[3], E.sub[4]) != 0)
        _DEV_CACHE[batch_family] = (b, E)
    return _DEV_CACHE[batch_family]


def _dev_flows(e, fst, b, E):
    """zkp_fused_prove_dev / _verify_compact_dev / _verify_batchable_dev / _batch_verify_dev on device buffers against E (the helper is shared with
    tests/test_gpu_random_statements.py, which runs it on other statements)"""
    SH.dev_flows(e, fst, b, E, names=_names(b))


@pytest.mark.parametrize("config", list(DEV_CONFIGS))
def test_dev_entry_points_on_every_schedule_and_term_path(config):
    b, E = _dev_case(None)
    e = EN.Engine(0)                                                       # a fresh context per configuration: no option has to be restored
    try:
        for opt, v in DEV_CONFIGS[config].items():
            e.set_option(opt, v)
        _dev_flows(e, _cmz_fst(), b, E)
    finally:
        e.close()


@pytest.mark.parametrize("fam", D.families_of("cmz10", "batch"))
@pytest.mark.parametrize("config", ["default", "latency", "grouped", "separate_terms"])
def test_dev_entry_points_with_degenerate_common_points(config, fam):
    b, E = _dev_case(fam)
    e = EN.Engine(0)
    try:
        for opt, v in DEV_CONFIGS[config].items():
            e.set_option(opt, v)
        _dev_flows(e, _cmz_fst(), b, E)
    finally:
        e.close()


# ---- CMZ on both sides of the thresholds that change the term path (tests/size_thresholds.py rows 6 and 8) ---------------------------------------
THRESHOLD_CASES = [(r, n) for r in __import__("tests.size_thresholds", fromlist=["ROWS"]).ROWS
                   if r["entry"] == "prove_cmz" and r["key"] in ("lat_split", "comb_min") and r["value"] in (8192, 250000) for n in r["sizes"]]


@pytest.mark.parametrize("r,n", THRESHOLD_CASES, ids=["%s-%s-%d" % (r["row"], r["name"], n) for r, n in THRESHOLD_CASES])
def test_cmz_degenerate_proofs_on_both_sides_of_the_term_path_thresholds(r, n):
    """prove and verify_compact through the _dev entry points at the default options; zkp_debug_last_schedule confirms the side.  The oracle
    recomputes the degenerate proofs and 32 ordinary ones.  Every ordinary proof is an honest proof of a true statement with non-identity
    points, which the protocol accepts with certainty: verify_compact may refuse degenerate proofs only, and those as the oracle says."""
    torch = _torch()
    assert len(THRESHOLD_CASES) == 4
    b = D.build_batch("cmz10", n, D.dense_plan("cmz10", n), n)
    _, cst = b.shape.build()
    rng = np.random.default_rng(n)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sample = sorted(set(b.degenerate) | {int(x) for x in rng.integers(0, n, size=32)})
    e = EN.Engine(0, test_hooks=True)
    try:
        e.set_option(EN.ZKP_OPT_DEV_OVERLAP, 2 if r["schedule"] == "latency" else 0)
        fst = _cmz_fst()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
        t0 = T.Transcript(b"degenerate").state
        pos = int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16
        ts0 = np.stack([t0] * n)
        e.prepare_fixed_points(b.common)
        d_tbl = dev(np.concatenate([b.common, b.inst.reshape(-1, 32)]))
        d_ts, d_sec, d_ent = dev(ts0), dev(b.secrets), dev(entropy)
        d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, 21, 32), z(n, 11, 32), z(11 * n)
        torch.cuda.synchronize()
        e.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                          d_coms.data_ptr(), d_st.data_ptr())
        e.synchronize()
        sched = e.last_schedule()
        assert sched.get(r["key"]) == r["expect"][r["sizes"].index(n)], sched
        assert not d_st.cpu().numpy().any()
        d_ts2, d_res = dev(ts0), z(n) + 7
        torch.cuda.synchronize()
        e.fused_verify_compact_dev(fst, n, pos, d_ts2.data_ptr(), d_tbl.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_res.data_ptr())
        e.synchronize()
        chal, resp, coms, res = d_chal.cpu().numpy(), d_resp.cpu().numpy(), d_coms.cpu().numpy(), d_res.cpu().numpy()
    finally:
        e.close()
    for j in sample:
        pts = D.points_of(b, j)
        ec, er, ek, _ = C.prove(cst, b"degenerate", b.secrets[j], pts, entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), "proof %d (%s) differs from the oracle's" % (j, _names(b).get(j, "ordinary"))
        assert res[j] == (C.verify_compact(cst, b"degenerate", pts, ec, er) != 0), "verdict of proof %d (%s)" % (j, _names(b).get(j, "ordinary"))
    assert set(np.nonzero(res)[0]) <= set(b.degenerate)


# ---- the seeded synchronous calls: entropy is drawn inside, so the oracle judges what they emit -------------------------------------------------------
def test_seeded_calls_emit_proofs_the_oracle_judges_like_its_own(eng):
    """zkp_fused_prove_seeded: every proof it emits for the dense CMZ batch goes to the ORACLE's verifiers and must get the verdict the oracle
    gives its own honest proof of the same inputs (E.vc / E.vb).  zkp_fused_batch_verify_many_seeded: the whole batch and the batch of the
    proofs the oracle accepts one by one get the oracle's verdicts."""
    hip = EN.load_library()
    b, E = _dev_case(None)
    n, fst = b.n, _cmz_fst()
    _, cst = b.shape.build()
    seed = bytes(range(11, 51))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ts = np.stack([T.Transcript(E.tl).state] * n)
    sec, ins, com = b.secrets.copy(), b.inst.copy(), b.common.copy()
    c2, r2, k2 = np.zeros((n, 32), np.uint8), np.zeros((n, 21, 32), np.uint8), np.zeros((n, 11, 32), np.uint8)
    invalid = ctypes.c_int(1)
    eng.prepare_fixed_points(com)
    rc = hip.zkp_fused_prove_seeded(eng._h, ctypes.byref(fst.c), ctypes.c_uint32(n), p(ts), p(sec), p(ins), p(com), seed, p(c2), p(r2), p(k2), ctypes.byref(invalid))
    assert rc == 0 and invalid.value == 0
    for j in range(n):
        pts = D.points_of(b, j)
        assert (C.verify_compact(cst, E.tl, pts, c2[j], r2[j]) != 0) == E.vc[j], "proof %d (%s)" % (j, _names(b).get(j, "ordinary"))
        assert (C.verify_batchable(cst, E.tl, pts, k2[j], r2[j], E.w_each[j]) != 0) == E.vb[j], "proof %d (%s)" % (j, _names(b).get(j, "ordinary"))
    acc = E.vb == 0
    sub = lambda a, axis=0: np.ascontiguousarray(np.compress(acc, a, axis=axis))
    for k, inst, coms, resp, want in ((n, ins, k2, r2, E.rc_batch), (int(acc.sum()), sub(ins, 1), sub(k2), sub(r2), E.rc_sub)):
        ts2 = np.stack([T.Transcript(E.tl).state] * k)
        verdicts = (ctypes.c_int * 1)(7)
        rc = hip.zkp_fused_batch_verify_many_seeded(eng._h, ctypes.byref(fst.c), ctypes.c_uint32(1), ctypes.c_uint32(k), p(ts2), p(inst), p(com), p(coms), p(resp), seed, verdicts)
        assert rc == 0 and verdicts[0] == want, (k, rc, verdicts[0], want)

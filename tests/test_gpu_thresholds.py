"""The default kernel selection on both sides of every size threshold (tests/size_thresholds.py), on the GPU.

For each row and each of its sizes:
* the boundary is really crossed: zkp_debug_last_schedule of the test-hook build reports the row's expected choice;
* the default bytes equal the bytes of every forced choice (zkp_ctx_set_option) and of the shipped library;
* the results are checked independently: MSM rows through points of known discrete logs (the sum of all outputs, the C oracle on a
  sample that always holds the first and the last output and positions 255 / 256, 65,535 / 65,536, 131,071 / 131,072 where present,
  identity outputs where MSMs were made to cancel), prove rows against the oracle's prover byte for byte, verify rows by rejecting
  exactly the planted mutants."""
import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests import size_thresholds as S

pytestmark = pytest.mark.gpu
BASE = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8).reshape(1, 32)
ZKP_CT, ZKP_VARTIME = 1, 0
OPT_DEV_OVERLAP = 5
N_RANDOM = 32                       # random outputs / proofs the oracle recomputes per call, besides the fixed positions


@pytest.fixture(scope="module")
def engines():
    """(test-hook engine, shipped engine)"""
    from zkp_amd.engine import Engine
    eh, es = Engine(0, test_hooks=True), Engine(0)
    yield eh, es
    eh.close()
    es.close()


def _forced(option, value, schedule=None):
    """a fresh test-hook engine with one option forced (a fresh context: ZKP_OPT_BATCH_ENCODE_MIN, once set, has no way back to its default)"""
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    if schedule == "latency":
        e.set_option(OPT_DEV_OVERLAP, 2)
    e.set_option(option, value)
    return e


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def _rand_scalars(rng, k):
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def _ints(arr):
    w = np.ascontiguousarray(arr).view(np.uint64).reshape(-1, 4)
    return [int(a) | (int(b) << 64) | (int(c) << 128) | (int(d) << 192) for a, b, c, d in w]


def _expected_point(total_log):
    return M.ristretto_encode(M.pt_mul(total_log % M.L, M.BASEPOINT))


def _total_log(scalars, pidx, logs):
    """sum_t s_t * log(P_pidx[t]) mod l, exactly: per point sums of 16-bit limbs (float64 bincount sums stay below 2^53)"""
    limbs = np.ascontiguousarray(scalars).view(np.uint16).reshape(-1, 16)
    n_pts = len(logs)
    per_pt = np.zeros(n_pts, dtype=object)
    for j in range(16):
        sj = np.bincount(pidx, weights=limbs[:, j].astype(np.float64), minlength=n_pts).astype(np.int64)
        per_pt = per_pt + (sj.astype(object) << (16 * j))
    return int(np.dot(per_pt, np.array(logs, dtype=object))) % M.L


_POOL = {}


def _points(eng, n):
    """n points k_j * B with their logs (cached: the rows share them); a sample is checked against the oracle"""
    have = _POOL.get("pts")
    if have is None or len(have[0]) < n:
        rng = np.random.default_rng(4242)
        n_make = max(n, 1 << 17)
        ks = _rand_scalars(rng, n_make)
        pts, st = eng.msm_many(np.arange(n_make + 1, dtype=np.uint32), ks, np.zeros(n_make, np.uint32), BASE, ZKP_VARTIME)
        assert not st.any()
        sample = np.array([0, n_make - 1] + list(rng.integers(0, n_make, size=6)))
        exp, _ = C.msm_many(np.arange(9, dtype=np.uint32), ks[sample], np.zeros(8, np.uint32), BASE, 0)
        assert (pts[sample] == exp).all()
        _POOL["pts"] = have = (pts, _ints(ks))
    return have[0][:n], have[1][:n]


def _sample_positions(n, rng):
    fixed = [0, n - 1] + [p for p in (255, 256, 65535, 65536, 131071, 131072) if p < n]
    return sorted(set(fixed) | set(rng.integers(0, n, size=N_RANDOM).tolist()))


# ---- MSM jobs ------------------------------------------------------------------------------------------------------------------------
def _msm_job(r, size, rng):
    """-> (off, scalars, pidx, n_points, flags, cancel positions) of the CSR job that puts the row's size where its unit says"""
    key = r["key"]
    if key in ("terms_split", "batch_encode", "enc_groups"):
        n_msm = size
        cancel = [] if key == "terms_split" else [p for p in (0, 255, 256, 65535, 65536, n_msm - 1) if p < n_msm]
        per = np.ones(n_msm, np.int64)
        per[cancel] = 2                                   # s * P + (l - s) * P: the identity (k_encode_finish's zflag branch)
        off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
        n_terms = int(off[-1])
        n_points = 64
        pidx = rng.integers(0, n_points, size=n_terms).astype(np.uint32)
        sc = _rand_scalars(rng, n_terms)
        for p in cancel:
            t = int(off[p])
            pidx[t + 1] = pidx[t]
            sc[t + 1] = np.frombuffer(((M.L - int.from_bytes(sc[t].tobytes(), "little")) % M.L).to_bytes(32, "little"), np.uint8)
        return off, sc, pidx, n_points, ZKP_VARTIME, cancel
    if key == "ladder_interleave":
        # `size` single-use points (variable time: each on the ladder) and 3 terms per MSM on 64 shared points
        n_single = size
        n_shared_terms = 3 * n_single
        n_terms = n_single + n_shared_terms
        pidx = np.empty(n_terms, np.uint32)
        pidx[0::4] = 64 + np.arange(n_single, dtype=np.uint32)
        shared = rng.integers(0, 64, size=n_shared_terms).astype(np.uint32)
        mask = np.ones(n_terms, bool)
        mask[0::4] = False
        pidx[mask] = shared
        off = np.arange(0, n_terms + 1, 4, dtype=np.uint32)
        return off, _rand_scalars(rng, n_terms), pidx, 64 + n_single, ZKP_VARTIME, []
    # constant-time term counts (rows 6 - 8): 3 of 4 terms on 64 shared points, every 4th on a point of its own; MSMs of 16 terms
    n_terms = size
    pidx = rng.integers(0, 64, size=n_terms).astype(np.uint32)
    single = np.arange(0, n_terms, 4)
    pidx[single] = 64 + np.arange(len(single), dtype=np.uint32)
    off = np.concatenate([np.arange(0, n_terms, 16), [n_terms]]).astype(np.uint32)
    return off, _rand_scalars(rng, n_terms), pidx, 64 + len(single), ZKP_CT, []


def _run_msm(eng, dev, off, sc, pidx, pts, flags):
    if not dev:
        out, st = eng.msm_many(off, sc, pidx, pts, flags)
        return out, st
    torch = _torch()
    n_msm, n_terms = len(off) - 1, len(sc)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_off, d_sc, d_pidx, d_pts = d(off.view(np.int32)), d(sc), d(pidx.view(np.int32)), d(pts)
    d_out = torch.zeros((n_msm, 32), dtype=torch.uint8, device="cuda:0")
    d_st = torch.ones(n_msm, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.msm_many_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), d_pidx.data_ptr(), d_pts.data_ptr(), len(pts), n_terms, flags, d_out.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


def _check_msm_row(engines, r, size):
    eh, es = engines
    rng = np.random.default_rng(size)
    off, sc, pidx, n_points, flags, cancel = _msm_job(r, size, rng)
    pts, logs = _points(eh, n_points)
    dev = r["entry"] == "msm_many_dev"
    out, st = _run_msm(eh, dev, off, sc, pidx, pts, flags)
    assert not st.any()
    sched = eh.last_schedule()
    assert sched.get(r["key"]) == r["expect"][r["sizes"].index(size)], sched
    # forced choices and the shipped library: the same bytes
    if r["option"]:
        opt, values = r["option"]
        for v in values:
            ef = _forced(opt, v)
            try:
                got, _ = _run_msm(ef, dev, off, sc, pidx, pts, flags)
            finally:
                ef.close()
            assert (got == out).all(), "option %d = %d changed the bytes" % (opt, v)
    got, _ = _run_msm(es, dev, off, sc, pidx, pts, flags)
    assert (got == out).all(), "the shipped library computes other bytes"
    # the cancelled MSMs encode the identity; the sum of all outputs is predicted by the discrete logs
    for p in cancel:
        assert not out[p].any(), "output %d should be the identity" % p
    ones = np.zeros((len(out), 32), np.uint8)
    ones[:, 0] = 1
    assert eh.msm_optional(ones, out) == _expected_point(_total_log(sc, pidx, logs))
    # the oracle on a sample of outputs
    pos = _sample_positions(len(off) - 1, rng)
    s_off, s_sc, s_pidx = [0], [], []
    for p in pos:
        a, b = int(off[p]), int(off[p + 1])
        s_sc.append(sc[a:b])
        s_pidx.append(pidx[a:b])
        s_off.append(s_off[-1] + b - a)
    s_pidx = np.concatenate(s_pidx)
    used, local = np.unique(s_pidx, return_inverse=True)
    exp, _ = C.msm_many(np.array(s_off, np.uint32), np.concatenate(s_sc), local.astype(np.uint32), pts[used], 1 if flags == ZKP_CT else 0)
    assert (out[pos] == exp).all(), [p for p, a, b in zip(pos, out[pos], exp) if (a != b).any()]


def _check_optional_row(engines, r, size):
    eh, es = engines
    rng = np.random.default_rng(size)
    pts, logs = _points(eh, 1024)
    pidx = rng.integers(0, 1024, size=size).astype(np.uint32)
    sc = _rand_scalars(rng, size)
    big = pts[pidx]
    got = eh.msm_optional(sc, big)
    sched = eh.last_schedule()
    assert sched.get(r["key"]) == r["expect"][r["sizes"].index(size)], sched
    assert got == _expected_point(_total_log(sc, pidx, logs))
    assert es.msm_optional(sc, big) == got, "the shipped library computes another point"


# ---- fused flows (DLEQ; CMZ for the riders of verify_compact) -----------------------------------------------------------------------
def _flow_batch(eng, which, n):
    """(FusedStatement, oracle statement or None, secrets, inst, common, m, nc) of n proofs"""
    import bench
    from zkp_amd.engine import FusedStatement
    rng = np.random.default_rng(n + {"cmz": 7, "w64": 11}.get(which, 0))
    if which == "cmz":
        st, mst, label = bench.cmz_statement(), M.cmz_statement(), b"CMZ cred show n=10"
    elif which == "w64":                 # Q = sum_{i < 64} x_i G_i: 65 points + 1 constraint = 66 operands per proof
        st, mst, label = bench.w64_statement(), None, b"w64"
    else:
        st, mst, label = bench.dleq_macro_statement(), M.dleq_statement(), b"DLEQ proof"
    secrets, inst, common = bench.make_instance(eng, st, n, rng)
    return (FusedStatement(label, *st), None if mst is None else C.Statement.from_model(mst), secrets, inst, common, len(st[0]), len(st[2]))


def _transcripts(n):
    from zkp_amd import toolbox as T
    t0 = T.Transcript(b"thresholds").state
    return np.stack([t0] * n), int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16


def _prove_dev(eng, fst, n, ts0, pos, secrets, table, entropy, m, nc):
    torch = _torch()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
    d_ts, d_sec, d_tbl, d_ent = d(ts0), d(secrets), d(table), d(entropy)
    d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, m, 32), z(n, nc, 32), z(nc * n)
    torch.cuda.synchronize()
    eng.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                        d_coms.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    assert not d_st.cpu().numpy().any()
    return d_chal.cpu().numpy(), d_resp.cpu().numpy(), d_coms.cpu().numpy()


def _mutants(n):
    """index 0, one in the last partial wavefront / block of 256, and N - 1"""
    last_block = (n - 1) // 256 * 256
    return sorted({0, last_block + (n - 1 - last_block) // 2, n - 1})


def _schedule(eng, r):
    eng.set_option(OPT_DEV_OVERLAP, 2 if r["schedule"] == "latency" else 0)


def _check_prove_row(engines, r, size):
    eh, es = engines
    n = size
    fst, cst, secrets, inst, common, m, nc = _flow_batch(es, "cmz" if r["entry"] == "prove_cmz" else "dleq", n)
    ts0, pos = _transcripts(n)
    rng = np.random.default_rng(n + 1)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    table = np.concatenate([common, inst.reshape(-1, 32)])
    _schedule(eh, r)
    _schedule(es, r)
    try:
        chal, resp, coms = _prove_dev(eh, fst, n, ts0, pos, secrets, table, entropy, m, nc)
        sched = eh.last_schedule()
        assert sched.get(r["key"]) == r["expect"][r["sizes"].index(size)], sched
        opt, values = r["option"]
        for v in values:
            ef = _forced(opt, v, r["schedule"])
            try:
                got = _prove_dev(ef, fst, n, ts0, pos, secrets, table, entropy, m, nc)
            finally:
                ef.close()
            assert all((a == b).all() for a, b in zip(got, (chal, resp, coms))), "option %d = %d changed the proofs" % (opt, v)
        got = _prove_dev(es, fst, n, ts0, pos, secrets, table, entropy, m, nc)
        assert all((a == b).all() for a, b in zip(got, (chal, resp, coms))), "the shipped library proves other bytes"
    finally:
        eh.set_option(OPT_DEV_OVERLAP, 0)
        es.set_option(OPT_DEV_OVERLAP, 0)
    for j in _sample_positions(n, rng):
        ec, er, ek, _ = C.prove(cst, b"thresholds", secrets[j], np.concatenate([inst[:, j], common]), entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), "proof %d differs from the oracle's" % j


def _check_verify_row(engines, r, size):
    eh, es = engines
    torch = _torch()
    n = size
    which = {"verify_compact": "cmz", "verify_batchable_w64": "w64"}.get(r["entry"], "dleq")
    fst, cst, secrets, inst, common, m, nc = _flow_batch(es, which, n)
    ts0, pos = _transcripts(n)
    rng = np.random.default_rng(n + 2)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    table = np.concatenate([common, inst.reshape(-1, 32)])
    chal, resp, coms = _prove_dev(es, fst, n, ts0, pos, secrets, table, entropy, m, nc)
    bad = resp.copy()
    mut = _mutants(n)
    bad[mut, 0, 0] ^= 1
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    w = rng.integers(0, 256, size=(n, nc, 16), dtype=np.uint8)

    def verify(eng, responses):
        d_ts, d_res = d(ts0), torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
        if r["entry"] == "verify_compact":
            d_tbl, d_chal, d_resp = d(table), d(chal), d(responses)
            torch.cuda.synchronize()
            eng.fused_verify_compact_dev(fst, n, pos, d_ts.data_ptr(), d_tbl.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_res.data_ptr())
        else:
            d_tbl, d_resp, d_w = d(np.concatenate([table, coms.reshape(-1, 32)])), d(responses), d(w)
            torch.cuda.synchronize()
            eng.fused_verify_batchable_dev(fst, n, pos, d_ts.data_ptr(), d_tbl.data_ptr(), d_resp.data_ptr(), d_w.data_ptr(), d_res.data_ptr())
        eng.synchronize()
        return d_res.cpu().numpy()

    _schedule(eh, r)
    _schedule(es, r)
    try:
        ok = verify(eh, resp)
        sched = eh.last_schedule()
        assert sched.get(r["key"]) == r["expect"][r["sizes"].index(size)], sched
        assert not ok.any(), np.nonzero(ok)[0][:8]
        got = verify(eh, bad)
        assert np.nonzero(got)[0].tolist() == mut
        if r["option"]:
            opt, values = r["option"]
            for v in values:
                ef = _forced(opt, v, r["schedule"])
                try:
                    assert (verify(ef, bad) == got).all(), "option %d = %d changed the verdicts" % (opt, v)
                finally:
                    ef.close()
        assert (verify(es, bad) == got).all(), "the shipped library gives other verdicts"
    finally:
        eh.set_option(OPT_DEV_OVERLAP, 0)
        es.set_option(OPT_DEV_OVERLAP, 0)


def _check_batch_row(engines, r, size):
    """row 3b: reject -> accept -> reject -> accept on ONE context, the two sizes alternating (stale status words would show)"""
    eh, es = engines
    torch = _torch()
    sizes = r["sizes"]
    runs = []
    for n in sizes:
        fst, cst, secrets, inst, common, _, _ = _flow_batch(es, "dleq", n)
        ts0, pos = _transcripts(n)
        rng = np.random.default_rng(n + 3)
        entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        table = np.concatenate([common, inst.reshape(-1, 32)])
        chal, resp, coms = _prove_dev(es, fst, n, ts0, pos, secrets, table, entropy, 1, 2)
        bad = resp.copy()
        bad[_mutants(n), 0, 0] ^= 1
        w = rng.integers(0, 256, size=(2, n, 16), dtype=np.uint8)
        runs.append((n, fst, ts0, pos, table, coms, resp, bad, w, inst, common))

    def batch(eng, run, responses):
        n, fst, ts0, pos, table, coms, _, _, w, _, _ = run
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        d_pts = torch.zeros((1 + 5 * n, 32), dtype=torch.uint8, device="cuda:0")
        d_pts[: 1 + 3 * n] = d(table)
        d_ts, d_coms, d_resp, d_w = d(ts0), d(coms), d(responses), d(w)
        d_out = torch.ones(32, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((2,), 5, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        eng.fused_batch_verify_dev(fst, n, pos, d_ts.data_ptr(), d_pts.data_ptr(), d_coms.data_ptr(), d_resp.data_ptr(), d_w.data_ptr(), d_out.data_ptr(), d_st.data_ptr())
        eng.synchronize()
        st = d_st.cpu().numpy()
        assert not st.any(), st
        return not d_out.cpu().numpy().any()           # accepted: the batch MSM is the identity

    i = sizes.index(size)
    order = [runs[i], runs[1 - i], runs[i], runs[1 - i]]
    for k, run in enumerate(order):
        for eng in (eh, es):
            assert batch(eng, run, run[7]) is False, "a batch with mutants was accepted (call %d, N = %d)" % (k, run[0])
            if eng is eh:
                sched = eh.last_schedule()
                assert sched.get(r["key"]) == r["expect"][sizes.index(run[0])], sched
            assert batch(eng, run, run[6]) is True, "a clean batch was rejected (call %d, N = %d)" % (k, run[0])
    # batch_verify_locate (shipped library, toolbox) names the mutants
    from zkp_amd import toolbox as T
    n, fst, ts0, pos, table, coms, resp, bad, w, inst, common = runs[i]
    mod = T.dleq_module()
    T.set_fused_min_batch(0)
    try:
        ok, res = T.batch_verify_locate(es, mod.statement, ts0.copy(), inst, common, coms, bad, w)
    finally:
        T.set_fused_min_batch(32)
    assert not ok and np.nonzero(res)[0].tolist() == _mutants(n)


RUNNERS = {"msm_many": _check_msm_row, "msm_many_dev": _check_msm_row, "msm_optional": _check_optional_row, "prove": _check_prove_row,
           "prove_cmz": _check_prove_row, "verify_compact": _check_verify_row, "verify_batchable": _check_verify_row,
           "verify_batchable_w64": _check_verify_row, "batch_verify": _check_batch_row}
CASES = [(r, n) for r in S.ROWS for n in r["sizes"]]


@pytest.mark.parametrize("r,size", CASES, ids=[S.row_id(r, n) for r, n in CASES])
def test_threshold(engines, r, size):
    if r["unreachable"]:
        pytest.skip("unreachable by a default call: " + r["unreachable"])
    RUNNERS[r["entry"]](engines, r, size)

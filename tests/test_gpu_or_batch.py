"""The batchable 1-of-k OR-proofs on the device (include/zkp_or_batch_mi355x.h, zkp_or_batch_toolbox.h) against the model of
tests/or_batch_model.py and the host backend: the same bytes, verdicts and coefficient vectors, on both sides of every size at which the
batch verifier's multiscalar sum changes path.

The sum has ns + N k (ni + nc) operands: 1 + 15 N for S2 (DLEQ: ns 1, ni 3, nc 2) at k = 3.  msm_optional_impl takes the term path up to
192 operands and the bucket method above, and changes its window at 2^12 and 2^13 operands (tests/size_thresholds.py), so SIZES is
N = 1 (16, term path), 12 (181, term path), 13 (196, first bucket run), 65 (976), 272 (4,081, below 2^12), 273 (4,096, at 2^12) and
547 (8,206, above 2^13); k = 1 and 64 run at N = 33 (64: 10,561 operands and the widest per-proof loop)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import or_batch_cases as B
from tests import or_proof_cases as C
from tests.test_gpu_device_entry import _dev, _torch
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 2**32 - 1
SIZES = (1, 12, 13, 65, 272, 273, 547)
MODEL_CHECK_MAX = 65                   # the model's group sum is pure Python


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _device_route():
    old = T.get_or_min_batch(), T.get_or_batch_min_batch()
    T.set_or_min_batch(0)
    T.set_or_batch_min_batch(0)
    yield
    T.set_or_min_batch(old[0])
    T.set_or_batch_min_batch(old[1])


def prove(c, eng):
    ts = c.transcripts.copy()
    coms, chal, resp, status = T.or_prove_batchable(eng, c.st, ts, c.secrets, c.real, c.inst, c.common, c.entropy)
    return ts, coms, chal, resp, status


@functools.lru_cache(maxsize=None)
def _big():
    """S2, k = 3, the largest size: the host backend's proofs, computed once and cut down"""
    c = C.case("S2", 3, max(SIZES))
    return (c,) + prove(c, None)


def big(n):
    c, ts, coms, chal, resp, status = _big()
    assert not status.any()
    return c.cut(n), ts[:n].copy(), coms[:n].copy(), chal[:n].copy(), resp[:n].copy()


# ---- 1. the prover ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", C.NAMES)
def test_device_proofs_equal_the_model_the_host_backend_and_or_prove(eng, name, k):
    c = C.case(name, k)
    ts, coms, chal, resp, status = prove(c, eng)
    mts, mcoms, mchal, mresp = B.model(name, k)
    assert not status.any() and (coms == mcoms).all() and (chal == mchal).all() and (resp == mresp).all() and (ts == mts).all()
    ots, ochal, oresp, ostatus = c.prove(eng)
    assert (ts == ots).all() and (chal == ochal).all() and (resp == oresp).all() and (status == ostatus).all()
    wide = C.case(name, k, 257)
    for a, b in zip(prove(wide, eng), prove(wide, None)):
        assert (a == b).all()


def test_the_provers_kernels_do_not_depend_on_the_secret_branch(eng):
    name, k, n = "S2", 3, 257
    eng.set_profiling(True)
    try:
        seen = []
        for real in (np.zeros(n), np.full(n, k - 1), np.arange(n) % k):
            c = C.Case(name, k, n, real=real)
            _, coms, chal, resp, status = prove(c, eng)
            names = eng.last_kernels()
            assert not status.any() and "zkp::k_or_assemble" in names.get("scalars", [])
            seen.append(names)
            assert T.or_batch_verify(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp)
        assert seen[0] == seen[1] == seen[2]
    finally:
        eng.set_profiling(False)


# ---- 2. the per-proof verifier ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("S1", 2), ("S2", 3), ("S3", 5)])
def test_verify_batchable_accepts_and_each_tampering_rejects_its_own_proof_only(eng, name, k):
    c = C.case(name, k)
    mts, coms, chal, resp = B.model(name, k)
    ts = c.transcripts.copy()
    assert not T.or_verify_batchable(eng, c.st, ts, c.inst, c.common, coms, chal, resp).any() and (ts == mts).all()
    for what, cm, ch, rs, inst, victim in B.tamperings(c, coms, chal, resp):
        res = T.or_verify_batchable(eng, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs)
        want = np.zeros(c.n, np.uint8)
        want[victim] = 1
        assert (res == want).all(), what


def test_verify_batchable_on_mixed_strobe_positions_agrees_with_the_host_backend(eng):
    c = C.Case("S3", 3, 65, ragged=True)
    ts, coms, chal, resp, status = prove(c, eng)
    hts, hcoms, hchal, hresp, _ = prove(c, None)
    assert not status.any() and (ts == hts).all() and (coms == hcoms).all() and (chal == hchal).all() and (resp == hresp).all()
    resp[9, 1, 0] = C._bump(resp[9, 1, 0])
    coms[40, 2, 0] = coms[41, 2, 0]
    dts, hts = c.transcripts.copy(), c.transcripts.copy()
    dres = T.or_verify_batchable(eng, c.st, dts, c.inst, c.common, coms, chal, resp)
    hres = T.or_verify_batchable(None, c.st, hts, c.inst, c.common, coms, chal, resp)
    want = np.zeros(65, np.uint8)
    want[[9, 40]] = 1
    assert (dres == want).all() and (hres == want).all() and (dts == hts).all()
    assert T.or_batch_verify(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp) is False


# ---- 3. the batch verifier ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_batch_verify_on_both_sides_of_every_path_change(eng, n):
    c, pts, coms, chal, resp = big(n)
    for pattern in B.WEIGHT_PATTERNS:
        w = B.weights(pattern, n, c.k, c.st.nc)
        ts = c.transcripts.copy()
        ok, co = T.or_batch_verify_coeffs(eng, c.st, ts, c.inst, c.common, coms, chal, resp, w)
        assert ok and (ts == pts).all(), pattern
        assert (co == B.model_coeffs("S2", c.k, chal, resp, w)).all(), pattern
    w = B.weights("random", n, c.k, c.st.nc)
    if n <= MODEL_CHECK_MAX:
        assert B.model_batch_verify("S2", c, coms, chal, resp, w)
    assert T.or_batch_verify(None, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp, w)
    bad = resp.copy()
    bad[n // 2, 1, 0] = C._bump(resp[n // 2, 1, 0])                   # canonical, hashed nowhere: only the sum notices
    for e in (eng, None):
        ok, res = T.or_batch_verify_locate(e, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, bad, w)
        want = np.zeros(n, np.uint8)
        want[n // 2] = 1
        assert not ok and (res == want).all()


@pytest.mark.parametrize("k", [1, 64])
def test_one_branch_and_the_most_branches(eng, k):
    c = C.Case("S2", k, 33)
    dev, host = prove(c, eng), prove(c, None)
    for a, b in zip(dev, host):
        assert (a == b).all()
    ts, coms, chal, resp, status = dev
    assert not status.any()
    w = B.weights("random", 33, k, c.st.nc)
    vts = c.transcripts.copy()
    assert not T.or_verify_batchable(eng, c.st, vts, c.inst, c.common, coms, chal, resp).any() and (vts == ts).all()
    ok, co = T.or_batch_verify_coeffs(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp, w)
    assert ok and (co == B.model_coeffs("S2", k, chal, resp, w)).all()
    bad = chal.copy()
    bad[32, k - 1] = C._bump(chal[32, k - 1])
    ok, res = T.or_batch_verify_locate(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, bad, resp, w)
    assert not ok and res[32] == 1 and res.sum() == 1


@pytest.mark.parametrize("name,k", [("S1", 2), ("S2", 3), ("S3", 5)])
def test_every_tampering_fails_the_batch_and_is_located(eng, name, k):
    c = C.case(name, k)
    _, coms, chal, resp = B.model(name, k)
    w = B.weights("random", c.n, k, c.st.nc)
    for what, cm, ch, rs, inst, victim in B.tamperings(c, coms, chal, resp):
        assert not T.or_batch_verify(eng, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs, w), what
        ok, res = T.or_batch_verify_locate(eng, c.st, c.transcripts.copy(), inst, c.common, cm, ch, rs, w)
        want = np.zeros(c.n, np.uint8)
        want[victim] = 1
        assert not ok and (res == want).all(), what


def test_both_sides_of_the_threshold_agree_and_the_kernels_say_which_ran(eng):
    c = C.case("S3", 3)
    _, coms, chal, resp = B.model("S3", 3)
    bad = resp.copy()
    bad[5, 0, 1] = C._bump(resp[5, 0, 1])
    w = B.weights("random", c.n, 3, c.st.nc)
    eng.set_profiling(True)
    try:
        verdicts = {}
        for side, threshold in (("device", 0), ("host", NEVER), ("device again", c.n), ("host again", c.n + 1)):
            T.set_or_batch_min_batch(threshold)
            eng.scalar_invert(np.ones((1, 32), np.uint8))             # (another call in between: last_kernels is the last call's)
            ok, co = T.or_batch_verify_coeffs(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, resp, w)
            ran = "zkp::k_or_batch_coeff" in eng.last_kernels().get("scalars", [])
            assert ran == side.startswith("device"), side
            verdicts[side] = (ok, co.tobytes(), T.or_batch_verify(eng, c.st, c.transcripts.copy(), c.inst, c.common, coms, chal, bad, w))
        assert len(set(verdicts.values())) == 1 and verdicts["device"][0] is True and verdicts["device"][2] is False
    finally:
        eng.set_profiling(False)


# ---- 4. the _dev forms ----------------------------------------------------------------------------------------------------------------------
def test_dev_forms_on_torch_tensors_equal_the_host_pointer_forms(eng):
    torch = _torch()
    name, k, n = "S2", 3, 65
    c, fst = C.case(name, k), C.fused_statement(name)
    ts, coms, chal, resp, status = prove(c, eng)
    w = B.weights("random", n, k, c.st.nc)
    d_sec, d_real, d_inst, d_com, d_ent, d_w = _dev(c.secrets), _dev(c.real), _dev(c.inst), _dev(c.common), _dev(c.entropy), _dev(w)
    z = lambda *s: torch.full(s, 0x55, dtype=torch.uint8, device="cuda:0")        # noqa: E731
    d_coms, d_chal, d_resp, d_status, d_res = z(n, k, c.st.nc, 32), z(n, k, 32), z(n, k, c.st.m, 32), z(n), z(n)
    d_verdict = torch.full((1,), 0x55555555, dtype=torch.int32, device="cuda:0")
    d_ts = _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_prove_batchable_dev(fst, k, n, d_ts.data_ptr(), d_sec.data_ptr(), d_real.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_ent.data_ptr(),
                               d_coms.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_status.data_ptr())
    eng.synchronize()
    assert (d_coms.cpu().numpy() == coms).all() and (d_chal.cpu().numpy() == chal).all() and (d_resp.cpu().numpy() == resp).all()
    assert (d_ts.cpu().numpy() == ts).all() and not d_status.cpu().numpy().any()
    d_ts2 = _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_verify_batchable_dev(fst, k, n, d_ts2.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_coms.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                                d_res.data_ptr())
    eng.synchronize()
    assert not d_res.cpu().numpy().any() and (d_ts2.cpu().numpy() == ts).all()
    d_ts3 = _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_batch_verify_dev(fst, k, n, d_ts3.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_coms.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                            d_w.data_ptr(), d_verdict.data_ptr())
    eng.synchronize()
    assert int(d_verdict.cpu().numpy()[0]) == 0 and (d_ts3.cpu().numpy() == ts).all()
    bumped = resp.copy()
    bumped[17, 2, 0] = C._bump(resp[17, 2, 0])
    d_bad, d_ts4 = _dev(bumped), _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_batch_verify_dev(fst, k, n, d_ts4.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_coms.data_ptr(), d_chal.data_ptr(), d_bad.data_ptr(),
                            d_w.data_ptr(), d_verdict.data_ptr())
    eng.synchronize()
    assert int(d_verdict.cpu().numpy()[0]) == 1
    eng.or_verify_batchable_dev(fst, k, n, _dev(c.transcripts).data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_coms.data_ptr(), d_chal.data_ptr(),
                                d_bad.data_ptr(), d_res.data_ptr())
    eng.synchronize()
    res = d_res.cpu().numpy()
    assert res[17] == 1 and res.sum() == 1


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_change_nothing(eng):
    import ctypes

    from zkp_amd.engine import ZkpError, _ptr
    c, fst = C.case("S1", 2, 33), C.fused_statement("S1")
    _, coms, chal, resp = B.model("S1", 2, 33)
    w = B.weights("random", 33, 2, 1)
    lib, h = eng._lib, eng._h

    def batch(k, n, ts, coms_ptr):
        verdict = ctypes.c_int(0x5a5a)
        inst = np.ascontiguousarray(np.resize(c.inst, (max(k, 1), 1, 33, 32)))
        rc = lib.zkp_or_batch_verify(h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(inst), _ptr(c.common), coms_ptr, _ptr(chal), _ptr(resp), _ptr(w),
                                     ctypes.byref(verdict), None)
        return rc, verdict.value

    ts = c.transcripts.copy()
    rc, v = batch(65, 33, ts, _ptr(coms))
    assert rc < 0 and v == 0x5a5a and (ts == c.transcripts).all()
    rc, v = batch(2, 33, ts, None)
    assert rc < 0 and v == 0x5a5a and (ts == c.transcripts).all()
    ts[3, 200] = 166
    before = ts.copy()
    rc, v = batch(2, 33, ts, _ptr(coms))
    assert rc < 0 and v == 0x5a5a and (ts == before).all()
    with pytest.raises(ZkpError):
        eng.or_verify_batchable(fst, ts, c.inst, c.common, coms, chal, resp)
    with pytest.raises(ZkpError):
        eng.or_prove_batchable(fst, ts, c.secrets, c.real, c.inst, c.common, c.entropy)
    assert (ts == before).all()
    rc, v = batch(2, 0, ts, _ptr(coms))
    assert rc == 0 and v == 0 and (ts == before).all()
    e = c.transcripts[:0].copy()
    out = eng.or_prove_batchable(fst, e, c.secrets[:0], c.real[:0], c.inst[:, :, :0], c.common, c.entropy[:0])
    assert out[0].shape == (0, 2, 1, 32) and out[1].shape == (0, 2, 32)
    assert eng.or_verify_batchable(fst, e, c.inst[:, :, :0], c.common, coms[:0], chal[:0], resp[:0]).shape == (0,)
    assert T.or_batch_verify(eng, c.st, e, c.inst[:, :, :0], c.common, coms[:0], chal[:0], resp[:0]) is True


# ---- 6. the example -------------------------------------------------------------------------------------------------------------------------
def test_the_tally_example_runs_as_a_child_process():
    """examples/vote_1_of_k_tally_batch.py 4096 on the device: the box passes, the box with two bad ballots fails, both are located, the tally
    is right"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "vote_1_of_k_tally_batch.py"), "4096"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "box of 4096 ballots: batch check passed" in lines and "box with 2 bad ballots: batch check failed" in lines
    assert "located: ballots 4096 and 4097" in lines
    cast = int(np.random.default_rng(4096).integers(0, 4, size=4096).sum())
    assert "tally: %d (cast: %d)" % (cast, cast) in lines

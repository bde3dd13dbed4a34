"""The batched 1-of-k OR-proofs on the device (include/zkp_or_mi355x.h, zkp_or_toolbox.h) against the model of tests/or_proof_model.py and
the host backend: the same bytes, the same verdicts, the same kernels whatever the secret branch is."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import or_proof_cases as C
from tests.test_gpu_device_entry import _dev, _torch
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 2**32 - 1


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _device_route():
    old = T.get_or_min_batch()
    T.set_or_min_batch(0)
    yield
    T.set_or_min_batch(old)


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("name", C.NAMES)
def test_device_proofs_equal_the_model_and_the_host_backend(eng, name, k):
    c = C.case(name, k)
    ts, chal, resp, status = c.prove(eng)
    mts, mchal, mresp = C.model(name, k)
    assert not status.any() and (chal == mchal).all() and (resp == mresp).all() and (ts == mts).all()
    vts, res = c.verify(eng, chal, resp)
    assert not res.any() and (vts == mts).all()
    big = C.case(name, k, 257)
    dev, host = big.prove(eng), big.prove(None)
    for a, b in zip(dev, host):
        assert (a == b).all()
    dv, hv = big.verify(eng, dev[1], dev[2]), big.verify(None, dev[1], dev[2])
    assert not dv[1].any() and not hv[1].any() and (dv[0] == hv[0]).all() and (dv[0] == dev[0]).all()


@pytest.mark.parametrize("k", [1, 64])
def test_one_branch_and_the_most_branches(eng, k):
    c = C.Case("S2", k, 33)
    dev, host = c.prove(eng), c.prove(None)
    for a, b in zip(dev, host):
        assert (a == b).all()
    assert not dev[3].any()
    vts, res = c.verify(eng, dev[1], dev[2])
    assert not res.any() and (vts == dev[0]).all()


@pytest.mark.parametrize("name,k", [("S1", 2), ("S2", 3), ("S3", 5)])
def test_each_tampering_rejects_its_own_proof_only(eng, name, k):
    c = C.case(name, k)
    _, chal, resp, _ = c.prove(eng)
    for what, ch, rs, inst, victim in C.tamperings(c, chal, resp):
        _, res = c.verify(eng, ch, rs, inst=inst)
        want = np.zeros(c.n, np.uint8)
        want[victim] = 1
        assert (res == want).all(), what


def test_dev_forms_on_torch_tensors_equal_the_host_pointer_forms(eng):
    torch = _torch()
    name, k, n = "S2", 3, 65
    c, fst = C.case(name, k), C.fused_statement(name)
    ts, chal, resp, status = c.prove(eng)
    d_ts, d_sec, d_real, d_inst = _dev(c.transcripts), _dev(c.secrets), _dev(c.real), _dev(c.inst)
    d_com, d_ent = _dev(c.common), _dev(c.entropy)
    z = lambda *s: torch.full(s, 0x55, dtype=torch.uint8, device="cuda:0")        # noqa: E731
    d_chal, d_resp, d_status, d_res = z(n, k, 32), z(n, k, c.st.m, 32), z(n), z(n)
    torch.cuda.synchronize()
    eng.or_prove_dev(fst, k, n, d_ts.data_ptr(), d_sec.data_ptr(), d_real.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_ent.data_ptr(),
                     d_chal.data_ptr(), d_resp.data_ptr(), d_status.data_ptr())
    eng.synchronize()
    assert (d_chal.cpu().numpy() == chal).all() and (d_resp.cpu().numpy() == resp).all() and (d_ts.cpu().numpy() == ts).all()
    assert not d_status.cpu().numpy().any()
    d_ts2 = _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_verify_dev(fst, k, n, d_ts2.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_res.data_ptr())
    eng.synchronize()
    assert not d_res.cpu().numpy().any() and (d_ts2.cpu().numpy() == ts).all()
    # a branch index of k or more: status 1 and zero rows for that proof alone
    real = c.real.copy()
    real[7] = k
    d_real = _dev(real)
    d_ts3 = _dev(c.transcripts)
    torch.cuda.synchronize()
    eng.or_prove_dev(fst, k, n, d_ts3.data_ptr(), d_sec.data_ptr(), d_real.data_ptr(), d_inst.data_ptr(), d_com.data_ptr(), d_ent.data_ptr(),
                     d_chal.data_ptr(), d_resp.data_ptr(), d_status.data_ptr())
    eng.synchronize()
    st = d_status.cpu().numpy()
    assert st[7] == 1 and st.sum() == 1 and not d_chal.cpu().numpy()[7].any() and not d_resp.cpu().numpy()[7].any()
    keep = np.arange(n) != 7
    assert (d_chal.cpu().numpy()[keep] == chal[keep]).all()


def test_the_toolbox_gives_the_same_bytes_on_both_sides_of_the_threshold(eng):
    c = C.case("S3", 3)
    T.set_or_min_batch(0)
    eng.set_profiling(True)
    try:
        dev = c.prove(eng)
        assert "zkp::k_or_respond" in eng.last_kernels().get("scalars", [])
        eng.scalar_invert(np.ones((1, 32), np.uint8))
        T.set_or_min_batch(NEVER)
        host = c.prove(eng)
        assert "zkp::k_or_respond" not in eng.last_kernels().get("scalars", [])
    finally:
        eng.set_profiling(False)
    for a, b in zip(dev, host):
        assert (a == b).all()
    assert (c.verify(eng, dev[1], dev[2])[1] == 0).all()
    T.set_or_min_batch(0)
    assert (c.verify(eng, dev[1], dev[2])[1] == 0).all()


def test_the_kernels_do_not_depend_on_the_secret_branch(eng):
    """zkp_ctx_last_kernels returns the same string for real all 0, all k - 1 and j mod k at equal shapes; every proof verifies"""
    name, k, n = "S2", 3, 257
    eng.set_profiling(True)
    try:
        seen = []
        for real in (np.zeros(n), np.full(n, k - 1), np.arange(n) % k):
            c = C.Case(name, k, n, real=real)
            _, chal, resp, status = c.prove(eng)
            names = eng.last_kernels()
            assert not status.any() and "zkp::k_or_assemble" in names.get("scalars", [])
            seen.append(names)
            assert not c.verify(eng, chal, resp)[1].any()
        assert seen[0] == seen[1] == seen[2]
    finally:
        eng.set_profiling(False)


def test_argument_errors_change_nothing(eng):
    from zkp_amd.engine import ZkpError
    c, fst = C.case("S1", 2, 33), C.fused_statement("S1")
    real = c.real.copy()
    real[5] = 2
    ts = c.transcripts.copy()
    with pytest.raises(ZkpError):
        eng.or_prove(fst, ts, c.secrets, real, c.inst, c.common, c.entropy)
    assert (ts == c.transcripts).all()
    ts[3, 200] = 166
    with pytest.raises(ZkpError):
        eng.or_prove(fst, ts, c.secrets, c.real, c.inst, c.common, c.entropy)
    chal, resp, status = eng.or_prove(fst, c.transcripts[:0].copy(), c.secrets[:0], c.real[:0], c.inst[:, :, :0], c.common, c.entropy[:0])
    assert chal.shape == (0, 2, 32)


def test_the_vote_example_runs_as_a_child_process():
    """examples/vote_1_of_k_batch.py 4096 on the device: every ballot accepted, both bad ballots rejected, the tally right"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "vote_1_of_k_batch.py"), "4096"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "ballots verified: 4096 of 4096" in lines and "v = 4 ballot: rejected" in lines and "tampered ballot: rejected" in lines
    cast = int(np.random.default_rng(4096).integers(0, 4, size=4096).sum())
    assert "tally: %d (cast: %d)" % (cast, cast) in lines

"""Batched Scalar * basepoint and Scalar * point on the MI355X: k_mul_base behind zkp_mul_base / _dev (the context's own fixed-base table of B,
crossbar look-up), k_mul_pairs<CT> behind zkp_mul_points / _dev (decode, signed radix-16 ladder, encode in one launch), and the toolbox
routing in front of them.  Checked against the oracle's C restatement, the host backend, and Engine.msm_many on the equivalent CSR job
(off = arange(n + 1), pidx = arange(n)) -- the route callers had before, whose code is unchanged.  Sizes sit on the wavefront and block
edges (63 / 64 / 65, 255 / 256 / 257), where crossbar lanes beyond n and partial blocks can go wrong; the operands are those of
tests/point_mul_cases.py, tiled."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

from oracle import cbind as C
from tests import point_mul_cases as PC
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT, ZKP_VARTIME

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096]
ERR_ARG = -2


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks():
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    yield e
    e.close()


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def iota(n):
    return np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32)


def gpu_pairs():
    """the pair operands with the invalid encodings (the last rows of the catalogue) rotated to the front, so that the smallest sizes hold
    them too: (scalars, points, expected out, expected status)"""
    s, p, _ = PC.pair_operands()
    want, st = PC.pair_expected()
    k = 6 * 7 + 3                                                      # (not a multiple of 3: a triple straddles the wrap)
    return tuple(np.roll(a, k, axis=0) for a in (s, p, want, st))


@pytest.mark.parametrize("n", SIZES)
def test_mul_base_equals_oracle_host_backend_and_msm_many(eng, n):
    s = PC.tiled(PC.base_operands(), n)
    want = PC.tiled(PC.base_expected(), n)
    got = eng.mul_base(s)
    assert (got == want).all()
    assert (got == T.basepoint_mul(None, s)).all()
    old, st = eng.msm_many(iota(n)[0], s, np.zeros(n, np.uint32), PC.BASEPOINT_ROW, ZKP_CT)
    assert (got == old).all() and not st.any()


@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
@pytest.mark.parametrize("n", SIZES)
def test_mul_points_equals_oracle_host_backend_and_msm_many(eng, n, flags):
    s, p, want, want_st = (PC.tiled(a, n) for a in gpu_pairs())
    if n >= 63:
        assert want_st.any() and not want_st.all()                     # invalid encodings among valid ones
    got, st = eng.mul_points(s, p, flags)
    assert (st == want_st).all()
    assert (got == want).all()                                         # (the neighbours of an invalid point included)
    assert not got[st == 1].any()
    host, host_st = T.point_mul(None, s, p, flags)
    assert (got == host).all() and (st == host_st).all()
    off, pidx = iota(n)
    old, old_st = eng.msm_many(off, s, pidx, p, flags)
    assert (got == old).all() and (st == old_st).all()


@pytest.mark.parametrize("ss,ps", list(itertools.product((0, 1), repeat=2)))
@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
def test_mul_points_strides(eng, ss, ps, flags):
    n = 257
    s, p, _, want_st = (PC.tiled(a, n) for a in gpu_pairs())
    p0 = int(np.flatnonzero(want_st == 0)[4])
    S = s if ss else s[9:10].copy()
    P = p if ps else p[p0:p0 + 1].copy()
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    rc = eng._lib.zkp_mul_points(eng._h, n, S.ctypes.data, ss, P.ctypes.data, ps, flags, out.ctypes.data, st.ctypes.data)
    assert rc == 0
    off, pidx = iota(n)
    want, wst = C.msm_many(off, s if ss else np.repeat(S, n, axis=0), pidx, p if ps else np.repeat(P, n, axis=0), 1)
    assert (out == want).all() and (st == wst).all()
    if ss or ps:                                                       # the wrapper derives the strides from the shapes
        got, gst = eng.mul_points(S if ss else S[0], P, flags)
        assert (got == out).all() and (gst == st).all()
    if not ps:                                                         # an invalid shared point fails every output
        got, gst = eng.mul_points(S, PC.enc_rows(PC.invalid_points()[3:4]), flags)
        assert gst.all() and not got.any()
    if ps:                                                             # out may be points
        buf, st2 = p.copy(), np.zeros(n, np.uint8)
        assert eng._lib.zkp_mul_points(eng._h, n, S.ctypes.data, ss, buf.ctypes.data, 1, flags, buf.ctypes.data, st2.ctypes.data) == 0
        assert (buf == want).all() and (st2 == wst).all()


def test_identities(eng):
    s = PC.tiled(PC.base_operands(), 300)
    out, st = eng.mul_points(s, PC.BASEPOINT_ROW)
    assert (out == eng.mul_base(s)).all() and not st.any()
    sc, p, _, bad = gpu_pairs()
    keep = (bad == 0) & np.array([int.from_bytes(bytes(r), "little") % PC.L != 0 for r in sc])
    sc, p = sc[keep], p[keep]
    sp, _ = eng.mul_points(sc, p)
    back, st = eng.mul_points(eng.scalar_invert(sc), sp)
    assert (back == p).all() and not st.any()
    assert not eng.mul_base(PC.rows([0, PC.L])).any()                  # the zero scalar: 32 zero bytes
    out, st = eng.mul_points(PC.rows([5, 0]), PC.enc_rows([PC.IDENTITY, PC.BASEPOINT]))
    assert not out.any() and not st.any()                              # the identity point / the zero scalar: zero bytes, status 0


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    s, p, _, _ = (PC.tiled(a, 4) for a in gpu_pairs())
    out, st = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    S, P, O, ST = s.ctypes.data, p.ctypes.data, out.ctypes.data, st.ctypes.data
    assert lib.zkp_mul_base(h, 0, None, None) == 0 and lib.zkp_mul_base_dev(h, 0, None, None) == 0
    assert lib.zkp_mul_points(h, 0, None, 1, None, 1, ZKP_CT, None, None) == 0
    assert lib.zkp_mul_points_dev(h, 0, None, 0, None, 0, ZKP_VARTIME, None, None) == 0
    assert lib.zkp_mul_base(None, 4, S, O) == ERR_ARG and lib.zkp_mul_points(None, 4, S, 1, P, 1, ZKP_CT, O, ST) == ERR_ARG
    assert lib.zkp_mul_base(h, 4, None, O) == ERR_ARG and lib.zkp_mul_base(h, 4, S, None) == ERR_ARG
    assert lib.zkp_mul_base_dev(h, 4, None, None) == ERR_ARG
    assert lib.zkp_mul_base(h, 2**31, S, O) == ERR_ARG and lib.zkp_mul_points(h, 2**31, S, 0, P, 0, ZKP_CT, O, ST) == ERR_ARG
    for args in ((None, 1, P, 1, ZKP_CT, O, ST), (S, 1, None, 1, ZKP_CT, O, ST), (S, 1, P, 1, ZKP_CT, None, ST), (S, 1, P, 1, ZKP_CT, O, None),
                 (S, 2, P, 1, ZKP_CT, O, ST), (S, 1, P, 2, ZKP_CT, O, ST), (S, 1, P, 1, 2, O, ST), (S, 1, P, 1, -1, O, ST)):
        assert lib.zkp_mul_points(h, 4, *args) == ERR_ARG, args
        assert lib.zkp_mul_points_dev(h, 4, *args) == ERR_ARG, args    # (rejected before any pointer is used)
    assert not out.any() and not st.any()


def test_profiling_names_the_kernels_under_terms(eng):
    s, p, _, _ = (PC.tiled(a, 200) for a in gpu_pairs())
    eng.set_profiling(True)
    try:
        eng.mul_base(s)
        assert eng.last_kernels() == {"terms": ["k_mul_base"]}
        ms, total = eng.last_timing()
        assert ms["terms"] > 0 and all(v == 0 for k, v in ms.items() if k != "terms")
        eng.mul_points(s, p, ZKP_CT)
        assert eng.last_kernels() == {"terms": ["k_mul_pairs<true>"]}
        eng.mul_points(s, p, ZKP_VARTIME)
        assert eng.last_kernels() == {"terms": ["k_mul_pairs<false>"]}
        assert eng.last_timing()[0]["terms"] > 0
    finally:
        eng.set_profiling(False)


def test_mul_base_takes_no_fixed_base_slot(hooks):
    """64 registered points fill every slot of zkp_ctx_prepare_fixed_points.  zkp_mul_base after that gives the oracle's bytes, and an
    msm_many over the 64 points makes the same choices and launches the same kernels before and after it: nothing was evicted."""
    rng = np.random.default_rng(64)
    ks = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    reg, _ = C.msm_many(iota(64)[0], ks, np.zeros(64, np.uint32), PC.BASEPOINT_ROW, 0)
    assert len({bytes(r) for r in reg}) == 64 and PC.BASEPOINT not in {bytes(r) for r in reg}
    hooks.prepare_fixed_points(reg)
    n_terms = 2048
    off = np.arange(0, n_terms + 1, 2, dtype=np.uint32)
    sc = rng.integers(0, 256, size=(n_terms, 32), dtype=np.uint8)
    pidx = (np.arange(n_terms) % 64).astype(np.uint32)
    hooks.set_profiling(True)
    try:
        before, st = hooks.msm_many(off, sc, pidx, reg, ZKP_CT)
        sched, kernels, tables_ms = hooks.last_schedule(), hooks.last_kernels(), hooks.last_timing()[0]["tables"]
        s = PC.tiled(PC.base_operands(), 300)
        assert (hooks.mul_base(s) == PC.tiled(PC.base_expected(), 300)).all()
        after, st2 = hooks.msm_many(off, sc, pidx, reg, ZKP_CT)
        assert hooks.last_schedule() == sched and hooks.last_kernels() == kernels
        assert (tables_ms == 0) == (hooks.last_timing()[0]["tables"] == 0)
    finally:
        hooks.set_profiling(False)
    assert (before == after).all() and not st.any() and not st2.any()
    want, _ = C.msm_many(off, sc, pidx, reg, 1)
    assert (after == want).all()


def test_results_do_not_depend_on_what_the_workspace_held():
    from zkp_amd.engine import Engine
    s, p, want, want_st = (PC.tiled(a, 700) for a in gpu_pairs())
    bs, bwant = PC.tiled(PC.base_operands(), 700), PC.tiled(PC.base_expected(), 700)
    e = Engine(0, test_hooks=True)
    try:
        for word in (0xFFFFFFFF, 3):
            e.debug_fill_workspace(8 << 20, word)
            assert (e.mul_base(bs) == bwant).all()
            for flags in (ZKP_CT, ZKP_VARTIME):
                e.debug_fill_workspace(8 << 20, word)
                got, st = e.mul_points(s, p, flags)
                assert (got == want).all() and (st == want_st).all()
    finally:
        e.close()


@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
def test_a_call_of_more_outputs_than_one_launch_holds_runs_in_pieces(eng, flags):
    """k_mul_pairs is launched over at most 262,144 lanes, which share the ladder tables; one output more makes a second piece of one lane.  The
    pieces' operand and output pointers advance by the strides.  k_mul_base at the same size is one launch with a partial last block."""
    n = 262144 + 1
    s, p, want, want_st = (PC.tiled(a, n) for a in gpu_pairs())
    got, st = eng.mul_points(s, p, flags)
    assert (got == want).all() and (st == want_st).all()
    k = len(gpu_pairs()[0])
    one, one_st = C.msm_many(iota(k)[0], np.repeat(s[7:8], k, axis=0), iota(k)[1], gpu_pairs()[1], 1)
    got, st = eng.mul_points(s[7], p, flags)                           # a shared scalar
    assert (got == PC.tiled(one, n)).all() and (st == PC.tiled(one_st, n)).all()
    pv = int(np.flatnonzero(want_st == 0)[2])
    one, _ = C.msm_many(iota(k)[0], gpu_pairs()[0], np.zeros(k, np.uint32), p[pv:pv + 1], 1)
    got, st = eng.mul_points(s, p[pv:pv + 1], flags)                   # a shared point
    assert (got == PC.tiled(one, n)).all() and not st.any()
    if flags == ZKP_CT:
        assert (eng.mul_base(PC.tiled(PC.base_operands(), n)) == PC.tiled(PC.base_expected(), n)).all()


def ragged_job(seed=5, n_msm=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, size=n_msm)
    lens[[0, 100]] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    t = int(off[-1])
    s, p, _, bad = gpu_pairs()
    pts = np.concatenate([p[bad == 0][:30], p[bad == 1][:1]])
    sc = s[rng.integers(0, len(s), size=t)]
    pidx = rng.integers(0, 30, size=t).astype(np.uint32)
    pidx[int(off[200])] = 30
    return off, np.ascontiguousarray(sc), pidx, np.ascontiguousarray(pts)


def test_toolbox_routes_to_the_device_and_equals_the_engine_calls(eng):
    assert T.get_host_max_terms() == 0                                 # (the gpu fixture: every size goes to the device)
    s, p, want, want_st = (PC.tiled(a, 65) for a in gpu_pairs())
    bs = PC.tiled(PC.base_operands(), 65)
    assert (T.basepoint_mul(eng, bs) == eng.mul_base(bs)).all()
    assert (T.basepoint_mul(eng, bs) == PC.tiled(PC.base_expected(), 65)).all()
    for flags in (ZKP_CT, ZKP_VARTIME):
        got, st = T.point_mul(eng, s, p, flags)
        ref, ref_st = eng.mul_points(s, p, flags)
        assert (got == ref).all() and (st == ref_st).all() and (got == want).all()
        got, st = T.point_mul(eng, s[0], p, flags)
        ref, ref_st = eng.mul_points(s[0], p, flags)
        assert (got == ref).all() and (st == ref_st).all()
        off, sc, pidx, pts = ragged_job()
        got, st = T.multiscalar_mul(eng, off, sc, pidx, pts, flags)
        ref, ref_st = eng.msm_many(off, sc, pidx, pts, flags)
        assert (got == ref).all() and (st == ref_st).all() and st.sum() == 1
        host, host_st = T.multiscalar_mul(None, off, sc, pidx, pts, flags)
        assert (got == host).all() and (st == host_st).all()
    # the other side of the routing threshold: at most host_max_terms outputs run on the host threads, same bytes
    T.set_host_max_terms(64)
    try:
        assert (T.basepoint_mul(eng, bs[:64]) == eng.mul_base(bs[:64])).all()
        got, st = T.point_mul(eng, s[:64], p[:64])
        assert (got == want[:64]).all() and (st == want_st[:64]).all()
    finally:
        T.set_host_max_terms(0)


def test_dev_forms_on_a_side_stream_and_recorded_into_a_graph():
    """zkp_mul_base_dev / zkp_mul_points_dev on torch device buffers, queued on a side stream, then recorded into a graph whose replay follows
    new inputs placed in the same buffers; d_out = d_points in the recorded zkp_mul_points_dev."""
    torch = _torch()
    from zkp_amd.engine import Engine
    n = 1000
    s, p, want, want_st = (PC.tiled(a, n) for a in gpu_pairs())
    bs, bwant = PC.tiled(PC.base_operands(), n), PC.tiled(PC.base_expected(), n)
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_s = torch.from_numpy(s).to("cuda:0")
    d_p = torch.from_numpy(p).to("cuda:0")
    d_bs = torch.from_numpy(bs).to("cuda:0")
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    d_bout = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    e.mul_base_dev(n, d_bs.data_ptr(), d_bout.data_ptr())
    e.mul_points_dev(n, d_s.data_ptr(), 1, d_p.data_ptr(), 1, ZKP_CT, d_out.data_ptr(), d_st.data_ptr())
    e.synchronize()
    assert (d_bout.cpu().numpy() == bwant).all()
    assert (d_out.cpu().numpy() == want).all() and (d_st.cpu().numpy() == want_st).all()
    e.mul_points_dev(n, d_s.data_ptr(), 0, d_p.data_ptr(), 1, ZKP_VARTIME, d_out.data_ptr(), d_st.data_ptr())
    e.synchronize()
    ref, ref_st = C.msm_many(iota(n)[0], np.repeat(s[:1], n, axis=0), iota(n)[1], p, 0)
    assert (d_out.cpu().numpy() == ref).all() and (d_st.cpu().numpy() == ref_st).all()
    d_bout.zero_()
    d_st.zero_()
    torch.cuda.synchronize()
    with e.capture() as cap:
        e.mul_base_dev(n, d_bs.data_ptr(), d_bout.data_ptr())
        e.mul_points_dev(n, d_s.data_ptr(), 1, d_p.data_ptr(), 1, ZKP_CT, d_p.data_ptr(), d_st.data_ptr())      # in place
    assert not bool(d_bout.any().item()) and bool((d_p.cpu() == torch.from_numpy(p)).all().item())               # recorded, not run
    cap.graph.launch()
    e.synchronize()
    assert (d_bout.cpu().numpy() == bwant).all()
    assert (d_p.cpu().numpy() == want).all() and (d_st.cpu().numpy() == want_st).all()
    # new inputs in the same buffers: the operands in reverse order
    d_bs.copy_(torch.from_numpy(bs[::-1].copy()).to("cuda:0"))
    d_s.copy_(torch.from_numpy(s[::-1].copy()).to("cuda:0"))
    d_p.copy_(torch.from_numpy(p[::-1].copy()).to("cuda:0"))
    torch.cuda.synchronize()
    cap.graph.launch()
    e.synchronize()
    assert (d_bout.cpu().numpy() == bwant[::-1]).all()
    assert (d_p.cpu().numpy() == want[::-1]).all() and (d_st.cpu().numpy() == want_st[::-1]).all()
    cap.graph.close()
    e.close()


def test_mul_base_dev_under_capture_needs_one_call_outside_it():
    torch = _torch()
    from zkp_amd.engine import Engine, ZkpError
    n = 64
    bs = PC.tiled(PC.base_operands(), n)
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_bs = torch.from_numpy(bs).to("cuda:0")
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    e.capture_begin()
    rc = e._lib.zkp_mul_base_dev(e._h, n, d_bs.data_ptr(), d_out.data_ptr())
    msg = e._lib.zkp_last_error().decode()
    e.capture_abort()
    assert rc == ERR_ARG and "outside the capture" in msg
    with pytest.raises(ZkpError):                                      # zkp_mul_points_dev: the workspace rule, as for every call that uses it
        with e.capture():
            e.mul_points_dev(n, d_bs.data_ptr(), 1, d_bs.data_ptr(), 1, ZKP_CT, d_out.data_ptr(), d_out.data_ptr())
    e.mul_base_dev(n, d_bs.data_ptr(), d_out.data_ptr())               # the context is usable again, and the table gets built
    e.synchronize()
    assert (d_out.cpu().numpy() == PC.tiled(PC.base_expected(), n)).all()
    d_out.zero_()
    torch.cuda.synchronize()
    with e.capture() as cap:
        e.mul_base_dev(n, d_bs.data_ptr(), d_out.data_ptr())
    cap.graph.launch()
    e.synchronize()
    assert (d_out.cpu().numpy() == PC.tiled(PC.base_expected(), n)).all()
    cap.graph.close()
    e.close()


def test_the_keygen_vrf_example_on_the_engine(eng):
    spec = importlib.util.spec_from_file_location("keygen_vrf_batch", os.path.join(ROOT, "examples", "keygen_vrf_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 256
    r = mod.run(eng, n, key=bytes(range(1, 33)))
    assert r["accepted"] == n and all(v == n for v in r["rejected"].values()) and len(r["rejected"]) == 4
    want_pk, _ = C.msm_many(iota(n)[0], r["sk"], np.zeros(n, np.uint32), PC.BASEPOINT_ROW, 1)
    want_g, _ = C.msm_many(iota(n)[0], r["sk"], iota(n)[1], r["H"], 1)
    assert (r["pk"] == want_pk).all() and (r["G"] == want_g).all()
    host = mod.run(None, n, key=bytes(range(1, 33)))                   # the same keys on the host backend: the same bytes
    assert (host["pk"] == r["pk"]).all() and (host["G"] == r["G"]).all()

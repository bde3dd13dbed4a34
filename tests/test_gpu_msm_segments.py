"""Multiscalar sums with long segments on the MI355X: zkp_msm_segments / _dev run zkp_msm_many's term path up to the per-term products and fold the
term axis in the levels of zkp_sum_points (k_sum_fold_parts, k_sum_fold<false>@2.., k_sum_encode), with the toolbox routing in front of them.
Every comparison is byte for byte and status for status against four things: the oracle's msm_many on the same job (tests/msm_segments_cases.py),
Engine.msm_many on the same job (the route callers had, whose code is unchanged), toolbox.multiscalar_sum(None, ...) on the host threads, and the
statuses.  Every case runs in constant and in variable time.  Segment lengths sit around the fold's group size G, which is read from
zkp_sum_points_group() and never written here: the fold has 2, 3 and 4 levels above G, G^2 / 2 and G^3 / 4 terms."""
import numpy as np
import pytest

from oracle import cbind as C
from tests import msm_segments_cases as MC
from tests import point_sum_cases as SC
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT, ZKP_VARTIME

pytestmark = pytest.mark.gpu
FLAGS = (ZKP_VARTIME, ZKP_CT)
ERR_ARG = -2
BAD_STATEMENT = -10


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def G(eng):
    g = int(eng._lib.zkp_sum_points_group())
    assert g >= 4 and g % 2 == 0
    return g


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def check(eng, name, off, sc, pidx, points, flags, old_route=True):
    want, want_st = MC.expected(name, off, sc, pidx, points, flags)
    got, st = eng.msm_segments(off, sc, points, pidx, flags)
    assert (st == want_st).all(), name
    assert (got == want).all(), name
    host, host_st = T.multiscalar_sum(None, off, sc, points, pidx, flags)
    assert (host == got).all() and (host_st == st).all(), name
    if old_route:
        pi = np.arange(int(off[-1]), dtype=np.uint32) if pidx is None else pidx
        old, old_st = eng.msm_many(off, sc, pi, points, flags)
        assert (old == got).all() and (old_st == st).all(), name
    return want, want_st


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("which", range(10))
def test_one_segment_of_every_length_around_the_level_edges(eng, G, which, flags):
    n = MC.single_lengths(G)[which]
    assert SC.plan_levels(n, G) == (1 if n <= G else 2 if n <= G * G // 2 else 3)
    off, sc, pidx, pts = MC.job([n], seed=n)
    check(eng, "single%d" % n, off, sc, pidx, pts, flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_ragged_job(eng, G, flags):
    off, sc, pidx, pts = MC.job(MC.ragged_lengths(G), seed=2)
    want, st = check(eng, "ragged", off, sc, pidx, pts, flags)
    empty = np.flatnonzero(np.diff(off.astype(np.int64)) == 0)
    assert len(empty) == 4 and not want[empty].any() and not st.any()


@pytest.mark.parametrize("flags", FLAGS)
def test_four_levels_with_points_shared_through_pidx(eng, G, flags):
    lens = MC.four_level_lengths(G)
    assert SC.plan_levels(sum(lens), G) == 4 and SC.plan_levels(G ** 3 // 4, G) == 3
    off, sc, pidx, pts = MC.job(lens, seed=7)
    want, st = check(eng, "four", off, sc, pidx, pts, flags)
    assert not st.any() and not want[2].any() and want[0].any() and want[1].any() and want[3].any()


@pytest.mark.parametrize("flags", FLAGS)
def test_invalid_encodings_flag_their_segments_and_no_other(eng, G, flags):
    off, sc, pidx, points, flagged = MC.with_invalid(G)
    want, st = check(eng, "invalid", off, sc, pidx, points, flags)
    assert np.flatnonzero(st).tolist() == flagged and not want[flagged].any()
    clean_off, clean_sc, clean_pidx, pts = MC.job(MC.ragged_lengths(G) + [3 * G + 7, 4, 0, 9], seed=3)
    clean, _ = MC.expected("invalid-clean", clean_off, clean_sc, clean_pidx, pts, flags)
    rest = [i for i in range(len(off) - 1) if i not in flagged]
    assert (want[rest] == clean[rest]).all()


@pytest.mark.parametrize("flags", FLAGS)
def test_scalar_and_point_special_cases(eng, G, flags):
    off, sc, pidx, pts, identity = MC.special_cases(G)
    want, st = check(eng, "special", off, sc, pidx, pts, flags)
    assert not st.any() and not want[identity].any() and want[2].any() and want[4].any()


@pytest.mark.parametrize("flags", FLAGS)
def test_without_pidx_term_t_uses_point_t(eng, G, flags):
    off, sc, pidx, pts = MC.job(MC.ragged_lengths(G), seed=2)
    want, want_st = MC.expected("ragged", off, sc, pidx, pts, flags)
    _, _, rows = MC.own_points(off, sc, pidx, pts)
    got, st = eng.msm_segments(off, sc, rows, None, flags)
    assert (got == want).all() and (st == want_st).all()
    got, st = T.multiscalar_sum(eng, off, sc, rows, None, flags)
    assert (got == want).all() and (st == want_st).all()
    out, ost = np.full((len(off) - 1, 32), 0xEE, np.uint8), np.full(len(off) - 1, 0xEE, np.uint8)
    assert eng._lib.zkp_msm_segments(eng._h, len(off) - 1, off.ctypes.data, sc.ctypes.data, None, rows.ctypes.data, len(rows) - 1, flags, out.ctypes.data,
                                     ost.ctypes.data) == ERR_ARG
    assert (out == 0xEE).all() and (ost == 0xEE).all()


@pytest.mark.parametrize("flags", FLAGS)
def test_registered_points_keep_their_bytes(G, flags):
    """a job of more than 1,024 terms (the classified term path, where registered points take the fixed-base walk) before and after
    zkp_ctx_prepare_fixed_points on eleven of its points"""
    from zkp_amd.engine import Engine
    off, sc, pidx, pts = MC.job([G + 1, 600, 0, 500, 3], seed=8)
    assert off[-1] >= 1024
    want, want_st = MC.expected("registered", off, sc, pidx, pts, flags)
    e = Engine(0)
    try:
        e.set_profiling(True)
        before, st = e.msm_segments(off, sc, pts, pidx, flags)
        assert (before == want).all() and (st == want_st).all()
        e.prepare_fixed_points(pts[2:13])
        after, st = e.msm_segments(off, sc, pts, pidx, flags)
        assert (after == want).all() and (st == want_st).all()
        names = e.last_kernels()
        assert names["terms"][0].startswith("k_terms_split<") and names["reduce"][0] == "k_sum_fold_parts"
    finally:
        e.close()


@pytest.mark.parametrize("flags", FLAGS)
def test_dev_form_on_torch_buffers(G, flags):
    """zkp_msm_segments_dev on torch device buffers with the outputs poisoned beforehand: with pidx, without (one row per term), and with an index
    out of range, which flags its segment and no other"""
    torch = _torch()
    from zkp_amd.engine import Engine
    off, sc, pidx, pts = MC.job(MC.ragged_lengths(G), seed=2)
    want, want_st = MC.expected("ragged", off, sc, pidx, pts, flags)
    n_msm, n_terms = len(off) - 1, int(off[-1])
    _, _, rows = MC.own_points(off, sc, pidx, pts)
    dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
    d_off, d_sc, d_pidx, d_pts, d_rows = dev(off), dev(sc), dev(pidx), dev(pts), dev(rows)
    d_out = torch.full((n_msm, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n_msm,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    e = Engine(0)
    try:
        e.msm_segments_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), d_pidx.data_ptr(), d_pts.data_ptr(), len(pts), n_terms, flags, d_out.data_ptr(), d_st.data_ptr())
        e.synchronize()
        assert (d_out.cpu().numpy() == want).all() and (d_st.cpu().numpy() == want_st).all()
        d_out.fill_(0xAB)
        d_st.fill_(0xAB)
        torch.cuda.synchronize()
        e.msm_segments_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), None, d_rows.data_ptr(), n_terms, n_terms, flags, d_out.data_ptr(), d_st.data_ptr())
        e.synchronize()
        assert (d_out.cpu().numpy() == want).all() and (d_st.cpu().numpy() == want_st).all()
        # without pidx the number of points must be the number of terms: refused, nothing enqueued
        with pytest.raises(Exception):
            e.msm_segments_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), None, d_rows.data_ptr(), n_terms - 1, n_terms, flags, d_out.data_ptr(), d_st.data_ptr())
        # an index out of range flags that segment and no other
        victim = 7                                                     # the 3 G + 5 segment
        wild = pidx.copy()
        wild[int(off[victim]) + G] = len(pts) + 5
        d_wild = dev(wild)
        d_out.fill_(0xAB)
        d_st.fill_(0xAB)
        torch.cuda.synchronize()
        e.msm_segments_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), d_wild.data_ptr(), d_pts.data_ptr(), len(pts), n_terms, flags, d_out.data_ptr(), d_st.data_ptr())
        e.synchronize()
        flagged, expect = want_st.copy(), want.copy()
        flagged[victim] = 1
        expect[victim] = 0
        assert (d_st.cpu().numpy() == flagged).all() and (d_out.cpu().numpy() == expect).all()
    finally:
        e.close()


@pytest.mark.parametrize("flags", FLAGS)
def test_results_do_not_depend_on_what_the_workspace_held(G, flags):
    from zkp_amd.engine import Engine
    off, sc, pidx, pts = MC.job(MC.ragged_lengths(G), seed=2)
    want, want_st = MC.expected("ragged", off, sc, pidx, pts, flags)
    e = Engine(0, test_hooks=True)
    try:
        for word in (0xFFFFFFFF, 3):
            e.debug_fill_workspace(8 << 20, word)
            got, st = e.msm_segments(off, sc, pts, pidx, flags)
            assert (got == want).all() and (st == want_st).all()
    finally:
        e.close()


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    off, sc, pidx, pts = MC.job([3, 0, 5], seed=4)
    out, st = np.full((3, 32), 0xEE, np.uint8), np.full(3, 0xEE, np.uint8)
    OF, SCp, PI, P, O, ST = (a.ctypes.data for a in (off, sc, pidx, pts, out, st))
    one, dec = np.array([1, 3, 3, 8], np.uint32), np.array([0, 5, 3, 8], np.uint32)
    assert lib.zkp_msm_segments(h, 0, None, None, None, None, 0, 0, None, None) == 0
    assert lib.zkp_msm_segments_dev(h, 0, None, None, None, None, 0, 0, 0, None, None) == 0
    assert lib.zkp_msm_segments(None, 3, OF, SCp, PI, P, len(pts), 0, O, ST) == ERR_ARG
    for flags in (2, -1):
        assert lib.zkp_msm_segments(h, 3, OF, SCp, PI, P, len(pts), flags, O, ST) == ERR_ARG
        assert lib.zkp_msm_segments_dev(h, 3, OF, SCp, PI, P, len(pts), 8, flags, O, ST) == ERR_ARG      # (rejected before any pointer is used)
        assert T.lib().zkp_multiscalar_sum_batch(h, 3, OF, SCp, PI, P, len(pts), flags, 0, O, ST) == BAD_STATEMENT
    for bad_off in (one, dec):
        assert lib.zkp_msm_segments(h, 3, bad_off.ctypes.data, SCp, PI, P, len(pts), 0, O, ST) == ERR_ARG
        assert T.lib().zkp_multiscalar_sum_batch(h, 3, bad_off.ctypes.data, SCp, PI, P, len(pts), 0, 0, O, ST) == BAD_STATEMENT
    assert lib.zkp_msm_segments(h, 3, OF, SCp, PI, P, int(pidx.max()), 0, O, ST) == ERR_ARG               # an index out of range
    assert T.lib().zkp_multiscalar_sum_batch(h, 3, OF, SCp, PI, P, int(pidx.max()), 0, 0, O, ST) == BAD_STATEMENT
    assert lib.zkp_msm_segments(h, 3, OF, SCp, None, P, len(pts), 0, O, ST) == ERR_ARG                    # no pidx: n_points must be the number of terms
    for args in ((None, SCp, PI, P), (OF, None, PI, P), (OF, SCp, PI, None)):
        assert lib.zkp_msm_segments(h, 3, *args, len(pts), 0, O, ST) == ERR_ARG
    assert lib.zkp_msm_segments(h, 3, OF, SCp, PI, P, len(pts), 0, None, ST) == ERR_ARG
    assert lib.zkp_msm_segments(h, 3, OF, SCp, PI, P, len(pts), 0, O, None) == ERR_ARG
    assert (out == 0xEE).all() and (st == 0xEE).all()


@pytest.mark.parametrize("flags", FLAGS)
def test_toolbox_routes_on_both_sides_of_the_fold_threshold(eng, G, flags):
    """a job whose longest segment is one below zkp_toolbox_get_msm_fold_min_segment() is zkp_msm_many (its reduce kernels), one at the threshold
    is the fold; the same bytes either way"""
    assert T.get_host_max_terms() == 0                                 # (the gpu fixture: every size goes to the device)
    thr = G + 8
    below = [3, thr - 1, 0, 2, thr - 1, 1]
    at = [3, thr - 1, 0, 2, thr, 0]
    assert sum(below) == sum(at)
    old = T.get_msm_fold_min_segment()
    eng.set_profiling(True)
    T.set_msm_fold_min_segment(thr)
    try:
        assert T.get_msm_fold_min_segment() == thr
        wants = {}
        for name, lens, reduce in (("route-below", below, ["k_reduce_encode"]), ("route-at", at, ["k_sum_fold_parts", "k_sum_fold<false>@2"])):
            off, sc, pidx, pts = MC.job(lens, seed=9)
            want, want_st = wants[name] = MC.expected(name, off, sc, pidx, pts, flags)
            got, st = T.multiscalar_sum(eng, off, sc, pts, pidx, flags)
            assert eng.last_kernels()["reduce"] == reduce, name
            assert (got == want).all() and (st == want_st).all(), name
            _, _, rows = MC.own_points(off, sc, pidx, pts)             # pidx = None: the toolbox supplies the arange on the zkp_msm_many route
            got, st = T.multiscalar_sum(eng, off, sc, rows, None, flags)
            assert eng.last_kernels()["reduce"] == reduce, name
            assert (got == want).all() and (st == want_st).all(), name
        assert (wants["route-below"][0][:4] == wants["route-at"][0][:4]).all()      # (the two jobs share their first four segments)
    finally:
        T.set_msm_fold_min_segment(old)
        eng.set_profiling(False)

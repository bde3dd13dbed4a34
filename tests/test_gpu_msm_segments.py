"""Multiscalar sums with long segments on the MI355X: zkp_msm_segments / _dev run zkp_msm_many's term path up to the per-term products and fold the
term axis in the levels of zkp_sum_points (k_sum_fold_parts, k_sum_fold<false>@2.., k_sum_encode), with the toolbox routing in front of them.
Every comparison is byte for byte and status for status against four things: the oracle's msm_many on the same job (tests/msm_segments_cases.py),
Engine.msm_many on the same job (the route callers had, whose code is unchanged), toolbox.multiscalar_sum(None, ...) on the host threads, and the
statuses.  Every case runs in constant and in variable time.  Segment lengths sit around the fold's group size G, which is read from
zkp_sum_points_group() and never written here: the fold has 2, 3 and 4 levels above G, G^2 / 2 and G^3 / 4 terms.

The second half runs the term path's classes behind the fold (terms_cfg::terms_only): single-use points (the ladder, single-use comb tables, the
constant-time ladder), all classes in one call, the _dev form's generic bounds, forced variants, the 8,192- and 250,000-term rules, a dirtied
workspace.  Each of those cases reads back which term kernel, table kernel and schedule words the call used and fails on any other."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cbind as C
from tests import msm_segments_cases as MC
from tests import point_sum_cases as SC
from zkp_amd import toolbox as T
from zkp_amd.engine import (ZKP_CT, ZKP_OPT_COMB_SPLIT, ZKP_OPT_COMB_TEETH, ZKP_OPT_CT_SINGLE_USE_TABLES, ZKP_OPT_GROUPED_COMB, ZKP_OPT_LADDER_INTERLEAVE,
                            ZKP_OPT_TABLES_LANE, ZKP_TESTOPT_WAVE_CYCLES, ZKP_VARTIME)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(eng):
    """a call that faulted leaves the device in error for every context of the process: the session ends there instead of launching the remaining
    cases on that card"""
    yield
    try:
        eng.synchronize()
    except Exception as e:                                   # noqa: BLE001 -- whatever the runtime reports
        pytest.exit("the shared context reports a GPU error; nothing further is started: %s" % e, returncode=3)


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


def check(eng, name, off, sc, pidx, points, flags, old_route=True, probe=None):
    """probe(eng) runs right after zkp_msm_segments, before any other call on the engine: what that call launched and chose"""
    want, want_st = MC.expected(name, off, sc, pidx, points, flags)
    got, st = eng.msm_segments(off, sc, points, pidx, flags)
    if probe:
        probe(eng)
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


# ==== the classified term path (1,024 terms or more) with the fold behind it: every term class, both entry forms =================================
# A job of 1,024 terms or more is classified (k_terms_split): terms on registered points walk the fixed-base tables, points with two or more cold uses
# get a comb table, single-use points take the ladder (variable time), a comb table of their own (constant time, comb_min = 1) or the constant-time
# ladder (ZKP_OPT_CT_SINGLE_USE_TABLES = 0; also what the host-pointer form picks by itself when NO cold point of the job has a second use).  The jobs
# above draw from 64 points, so they only ever reach the comb-table class.  Every case below says which kernel instantiation, table kernel and schedule
# words it must have reached and fails when the call ran anything else.  The thresholds come from tests/size_thresholds.py.
TERMS_SPLIT = MC.threshold("n_terms >= 1024")
SPLIT_COMB = MC.threshold("kSplitCombTerms")
ENCODE_MIN = MC.threshold("kThroughputEncodeMin")
WIDE_CALL = MC.threshold("kWideCallTerms")
FOLD = "k_sum_fold_parts"
WS_FILL = 64 << 20             # many times what the largest job of the dirtied-workspace case carves (1,400 constant-time terms with 16 teeth: 12 MB)


@pytest.fixture(scope="module")
def prof():
    """the shipped library with profiling on (zkp_ctx_last_kernels); the toolbox takes contexts of this library only"""
    from zkp_amd.engine import Engine
    e = Engine(0)
    e.set_profiling(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks():
    """the test-hook build with profiling on: zkp_ctx_last_kernels and zkp_debug_last_schedule"""
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    e.set_profiling(True)
    yield e
    e.close()


def _new_hooks():
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    e.set_profiling(True)
    return e


def _seen(e):
    return e.last_kernels(), (e.last_schedule() if e.test_hooks else None)


def _term_args(kernels):
    """(CT, TEETH, ladder, LOOKUP, split) of the one term kernel the call launched, as the strings of its name"""
    names = kernels.get("terms", [])
    assert len(names) == 1 and names[0].startswith("k_terms_split<") and names[0].endswith(">"), kernels
    args = tuple(a.strip() for a in names[0][len("k_terms_split<"):-1].split(","))
    assert len(args) == 5, names
    return args


def classified_and_folded(kernels, sched, flags):
    """the call classified its terms, never halved its scalars and folded `part`; -> the term kernel's template arguments"""
    args = _term_args(kernels)
    assert args[0] == ("true" if flags == ZKP_CT else "false"), kernels
    assert kernels["reduce"][0] == FOLD, kernels
    if sched is not None:
        assert sched.get("terms_split") == 1 and sched.get("batch_encode") == 0, sched
    return args


def _dev_call(e, off, sc, pidx, points, flags, entry="segments", probe=None, stream=None):
    """zkp_msm_segments_dev (or zkp_msm_many_dev) on torch buffers, the outputs poisoned beforehand -> (out, status)"""
    torch = _torch()
    dev = lambda a: torch.from_numpy(np.array(a).view(np.int32) if a.dtype == np.uint32 else np.array(a)).to("cuda:0")
    n_msm, n_terms = len(off) - 1, int(off[-1])
    d_off, d_sc, d_pts = dev(off), dev(sc), dev(points)
    d_pidx = None if pidx is None else dev(pidx)
    d_out = torch.full((n_msm, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n_msm,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if stream is not None:
        e.set_stream(stream.cuda_stream)
    call = e.msm_segments_dev if entry == "segments" else e.msm_many_dev
    call(n_msm, d_off.data_ptr(), d_sc.data_ptr(), None if d_pidx is None else d_pidx.data_ptr(), d_pts.data_ptr(), len(points), n_terms, flags,
         d_out.data_ptr(), d_st.data_ptr())
    if probe:
        probe(e)
    e.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


# ---- a. own rows (pidx = NULL) around the edge of the classified path: every point has one use ---------------------------------------------------
def own_rows_path(form, kernels, sched, n_terms, flags):
    if form == "toolbox" and n_terms < T.get_msm_fold_min_segment():   # (1,024 by default: the toolbox sends shorter segments to zkp_msm_many)
        assert n_terms < TERMS_SPLIT and kernels == {"reduce": ["k_reduce_encode"]}, kernels
        return
    assert kernels["reduce"][0] == FOLD, kernels
    if n_terms < TERMS_SPLIT:                                          # one k_terms_r4 lane per term: nothing is classified
        assert "terms" not in kernels and (sched is None or sched.get("terms_split") == 0), (kernels, sched)
        return
    _, teeth, ladder, _, split = classified_and_folded(kernels, sched, flags)
    comb_min = None if sched is None else sched.get("comb_min")
    if flags == ZKP_VARTIME:                                           # the ladder class: groups of 64 wave-interleaved ladder tables
        assert ladder == "true" and comb_min in (None, 2), (form, kernels, sched)
    elif form == "dev":                                                # generic bounds of the throughput schedule: a 4-teeth comb table per row
        assert ladder == "false" and teeth == "4" and comb_min == 1 and kernels.get("tables") == ["zkp::k_comb_tables_lane<4>"], (form, kernels, sched)
    else:
        # the host-pointer form counts the uses (host_terms_cfg): a job without any cold point of two uses has no table chains to run the single-use tables
        # next to, so it sends the single-use points down the CONSTANT-TIME LADDER (comb_min 2, no table kernel)
        assert ladder == "true" and comb_min in (None, 2) and "tables" not in kernels, (form, kernels, sched)
    assert split == "false"


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("delta", (-1, 0, 1, 63, 64, 65))
def test_own_rows_around_the_edge_of_the_classified_path(prof, hooks, delta, flags):
    """one segment of T terms with a row per term, T = 1,023 (the k_terms_r4 side), 1,024 (16 full groups of 64 ladder tables), 1,025 (a group of one),
    1,087 (a group of 63), 1,088, 1,089: host-pointer form, toolbox route and _dev form (k_iota writes the index)"""
    n_terms = TERMS_SPLIT + delta
    off, sc, rows, _ = MC.own_rows_job(n_terms, seed=n_terms)
    seen = {}
    want, want_st = check(hooks, "own%d" % n_terms, off, sc, None, rows, flags, probe=lambda e: seen.update(host=_seen(e)))
    got, st = T.multiscalar_sum(prof, off, sc, rows, None, flags)
    seen["toolbox"] = _seen(prof)
    assert (got == want).all() and (st == want_st).all()
    got, st = _dev_call(hooks, off, sc, None, rows, flags, probe=lambda e: seen.update(dev=_seen(e)))
    assert (got == want).all() and (st == want_st).all()
    assert sorted(seen) == ["dev", "host", "toolbox"]
    for form, (kernels, sched) in seen.items():
        own_rows_path(form, kernels, sched, n_terms, flags)


# ---- b. registered, shared, twice-used and single-use points in one call ---------------------------------------------------------------------------
def _wave_classes(e):
    """the block classes of the term kernel that ran since the last read: 1 ladder, 2 comb scan, 3 grouped walk, 4 fixed-base (ZKP_TESTOPT_WAVE_CYCLES)"""
    cls, _ = e.debug_wave_cycles()
    return sorted(set(cls.tolist()))


@pytest.mark.parametrize("flags", FLAGS)
def test_all_four_term_classes_in_one_call(G, flags):
    """mixed_job before and after zkp_ctx_prepare_fixed_points on its 11 registered rows, then with an undecodable row in three of the classes.  The
    per-wavefront recorder of the test-hook build names the block classes that ran: the fixed-base blocks appear with the registration.  Teeth: the
    host-pointer form picks 16 where the table points carry two terms each on average (pick_teeth): 1,382 terms on 581 tables before the
    registration in constant time; 1,036 cold terms on 569 tables after it, which is 4"""
    off, sc, pidx, points, info = MC.mixed_job(G, TERMS_SPLIT + 1)
    name = "mixed%d" % (TERMS_SPLIT + 1)
    ct = flags == ZKP_CT
    ladder_blocks = [] if ct else [1]
    e = _new_hooks()
    try:
        e.set_option(ZKP_TESTOPT_WAVE_CYCLES, 1)
        seen = []
        probe = lambda x: seen.append(_seen(x) + (_wave_classes(x),))
        e.debug_wave_cycles()
        want, want_st = check(e, name, off, sc, pidx, points, flags, probe=probe)
        assert not want_st.any() and not want[info["identity"]].any()
        e.prepare_fixed_points(points[list(info["registered"])])
        e.debug_wave_cycles()
        got, st = e.msm_segments(off, sc, points, pidx, flags)
        probe(e)
        assert (got == want).all() and (st == want_st).all()
        (k0, s0, w0), (k1, s1, w1) = seen
        a0, a1 = classified_and_folded(k0, s0, flags), classified_and_folded(k1, s1, flags)
        assert w0 == ladder_blocks + [2] and w1 == ladder_blocks + [2, 4], (w0, w1)
        assert a0[1:3] == ("16", "false" if ct else "true") and a1[1:3] == ("4" if ct else "16", "false" if ct else "true"), (a0, a1)
        assert s0.get("comb_min") == s1.get("comb_min") == (1 if ct else 2) and s0.get("grouped") == 0 and s0.get("lat_split") == 0, (s0, s1)
        assert k0["tables"] == ["zkp::k_comb_tables<16>"] and k1["tables"] == ["zkp::k_comb_tables<%d>" % (4 if ct else 16)], (k0, k1)
        # an undecodable row in the shared, the twice-used and the single-use class: exactly their segments are flagged
        b_off, b_sc, b_pidx, b_points, flagged, _ = MC.mixed_job_with_invalid(G, TERMS_SPLIT + 1)
        e.debug_wave_cycles()
        bad, bad_st = check(e, "mixed-invalid", b_off, b_sc, b_pidx, b_points, flags, probe=probe)
        assert np.flatnonzero(bad_st).tolist() == flagged and not bad[flagged].any()
        rest = [i for i in range(len(off) - 1) if i not in flagged]
        assert (bad[rest] == want[rest]).all()
        classified_and_folded(seen[2][0], seen[2][1], flags)
        assert seen[2][2] == ladder_blocks + [2, 4], seen[2][2]
    finally:
        e.set_option(ZKP_TESTOPT_WAVE_CYCLES, 0)
        e.close()


# ---- c. forced variants -----------------------------------------------------------------------------------------------------------------------------
VARIANTS = [(n, o, v) for n, o, vals in (("COMB_TEETH", ZKP_OPT_COMB_TEETH, (4, 16)), ("CT_SINGLE_USE_TABLES", ZKP_OPT_CT_SINGLE_USE_TABLES, (0, 1)),
                                         ("GROUPED_COMB", ZKP_OPT_GROUPED_COMB, (0, 1)), ("TABLES_LANE", ZKP_OPT_TABLES_LANE, (0, 1)),
                                         ("LADDER_INTERLEAVE", ZKP_OPT_LADDER_INTERLEAVE, (0, 1)), ("COMB_SPLIT", ZKP_OPT_COMB_SPLIT, (0, 1))) for v in vals]
_DEFAULT = {}


def variant_path(option, value, form, kernels, sched, flags):
    _, teeth, ladder, _, split = classified_and_folded(kernels, sched, flags)
    ct = flags == ZKP_CT
    assert teeth == ("16" if form == "host" else str(value) if option == "COMB_TEETH" else "4"), (form, kernels)     # host: pick_teeth; dev: the option (default 4)
    single_use_tables = ct and not (option == "CT_SINGLE_USE_TABLES" and value == 0)
    assert ladder == ("false" if single_use_tables else "true") and sched.get("comb_min") == (1 if single_use_tables else 2), (form, kernels, sched)
    lane = value if option == "TABLES_LANE" else (1 if form == "dev" else 0)
    assert kernels["tables"] == ["zkp::k_comb_tables%s<%s>" % ("_lane" if lane else "", teeth)], (form, kernels)
    split_on = option == "COMB_SPLIT" and value == 1
    assert sched.get("lat_split") == (1 if split_on else 0), sched
    assert sched.get("grouped") == (value if option == "GROUPED_COMB" else 1 if split_on else 0), sched
    assert split == ("true" if split_on and ct and teeth == "16" and ladder == "false" else "false"), (form, kernels)
    if ladder == "true":
        assert sched.get("ladder_interleave") == (value if option == "LADDER_INTERLEAVE" else 0), sched
    else:
        assert "ladder_interleave" not in sched, sched


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("variant", VARIANTS, ids=["%s=%d" % (n, v) for n, _, v in VARIANTS])
def test_forced_variants_with_the_fold_behind_them(eng, G, variant, flags):
    """mixed_job on a fresh context per option value, host-pointer and _dev form: the oracle's bytes, the default context's bytes, and the variant the
    option names really ran"""
    from zkp_amd.engine import ZkpError
    option, number, value = variant
    off, sc, pidx, points, _ = MC.mixed_job(G, TERMS_SPLIT + 1)
    if flags not in _DEFAULT:
        _DEFAULT[flags] = eng.msm_segments(off, sc, points, pidx, flags)
    e = _new_hooks()
    try:
        try:
            e.set_option(number, value)
        except ZkpError as err:
            pytest.skip("this build refuses ZKP_OPT_%s = %d: %s" % (option, value, err))
        seen = {}
        want, want_st = check(e, "mixed%d" % (TERMS_SPLIT + 1), off, sc, pidx, points, flags, probe=lambda x: seen.update(host=_seen(x)))
        got, st = _dev_call(e, off, sc, pidx, points, flags, probe=lambda x: seen.update(dev=_seen(x)))
        assert (got == want).all() and (st == want_st).all()
        assert (_DEFAULT[flags][0] == want).all() and (_DEFAULT[flags][1] == want_st).all()
        for form in ("host", "dev"):
            variant_path(option, value, form, seen[form][0], seen[form][1], flags)
    finally:
        e.close()


# ---- d. the 8,192-term rule of the latency schedule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", (0, 1), ids=("below", "at"))
def test_quad_split_scans_and_grouped_walk_from_8192_terms(hooks, G, side):
    """constant time, host-pointer form: at kSplitCombTerms terms the comb scans go to quads of lanes and the points with many uses to the grouped walk"""
    total = SPLIT_COMB - 1 + side
    off, sc, pidx, points, _ = MC.mixed_job(G, total)
    assert int(off[-1]) == total
    seen = {}
    want, want_st = check(hooks, "mixed%d" % total, off, sc, pidx, points, ZKP_CT, probe=lambda e: seen.update(host=_seen(e)))
    kernels, sched = seen["host"]
    args = classified_and_folded(kernels, sched, ZKP_CT)
    assert sched.get("lat_split") == side and sched.get("grouped") == side and sched.get("comb_min") == 1, sched
    assert args[1:] == ("16", "false", "0", "true" if side else "false"), args
    e = _new_hooks()
    try:
        e.set_option(ZKP_OPT_COMB_SPLIT, 0)
        got, st = e.msm_segments(off, sc, points, pidx, ZKP_CT)
        k0, s0 = _seen(e)
        assert classified_and_folded(k0, s0, ZKP_CT)[4] == "false" and s0.get("lat_split") == 0, (k0, s0)
        assert (got == want).all() and (st == want_st).all()
    finally:
        e.close()


# ---- e. many short segments on the _dev form: zkp_msm_many_dev halves its scalars from 2,048 outputs on, the fold must not --------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("side", (0, 1), ids=("below", "at"))
def test_many_short_segments_never_run_on_halved_scalars(hooks, side, flags):
    n_msm = ENCODE_MIN - 1 + side
    off, sc, pidx, points = MC.many_segments_job(n_msm)
    assert int(off[-1]) >= TERMS_SPLIT
    want, want_st = MC.expected("many%d" % n_msm, off, sc, pidx, points, flags)
    seen = {}
    got, st = _dev_call(hooks, off, sc, pidx, points, flags, probe=lambda e: seen.update(fold=_seen(e)))
    assert (st == want_st).all() and (got == want).all()
    classified_and_folded(seen["fold"][0], seen["fold"][1], flags)
    old, old_st = _dev_call(hooks, off, sc, pidx, points, flags, entry="many", probe=lambda e: seen.update(many=_seen(e)))
    assert seen["many"][1].get("batch_encode") == side and seen["many"][1].get("terms_split") == 1, seen["many"]
    assert FOLD not in seen["many"][0].get("reduce", []), seen["many"]
    assert (old_st == want_st).all() and (old == want).all()


# ---- f. the _dev form at 1,024 terms or more, on a side stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_dev_form_on_the_classified_path(G, flags):
    """generic bounds of the throughput schedule (teeth = ZKP_OPT_COMB_TEETH, a table slot for every point, k_comb_tables_lane): the mixed job through
    d_pidx, the own-rows job with NULL, and an index out of range in a single-use term"""
    torch = _torch()
    from zkp_amd.engine import Engine
    off, sc, pidx, points, info = MC.mixed_job(G, TERMS_SPLIT + 1)
    want, want_st = MC.expected("mixed%d" % (TERMS_SPLIT + 1), off, sc, pidx, points, flags)
    n_own = TERMS_SPLIT + 65
    o_off, o_sc, o_rows, _ = MC.own_rows_job(n_own, seed=n_own)
    o_want, o_want_st = MC.expected("own%d" % n_own, o_off, o_sc, None, o_rows, flags)
    ct = flags == ZKP_CT
    e = Engine(0)
    try:
        e.set_profiling(True)
        stream = torch.cuda.Stream()
        seen = {}
        got, st = _dev_call(e, off, sc, pidx, points, flags, probe=lambda x: seen.update(mixed=_seen(x)), stream=stream)
        assert (st == want_st).all() and (got == want).all()
        got, st = _dev_call(e, o_off, o_sc, None, o_rows, flags, probe=lambda x: seen.update(own=_seen(x)))
        assert (st == o_want_st).all() and (got == o_want).all()
        for kernels, _ in seen.values():
            args = classified_and_folded(kernels, None, flags)
            assert args[1:3] == ("4", "false" if ct else "true") and kernels["tables"] == ["zkp::k_comb_tables_lane<4>"], kernels
        # an index out of range in a single-use term flags that segment and no other
        seg_of = lambda t: int(np.searchsorted(off, t, side="right")) - 1
        t = next(int(t) for t in np.flatnonzero(info["cls"] == MC.CLASS_ONCE)[40:]
                 if t != info["t_hot"] and seg_of(t) not in info["identity"] and off[seg_of(t)] < t < off[seg_of(t) + 1] - 1)
        victim = seg_of(t)
        assert want[victim].any()
        wild = pidx.copy()
        wild[t] = len(points) + 5
        got, st = _dev_call(e, off, sc, wild, points, flags)
        flagged, expect = want_st.copy(), want.copy()
        flagged[victim] = 1
        expect[victim] = 0
        assert (st == flagged).all() and (got == expect).all()
    finally:
        e.close()


# ---- g. the classified path behind a dirtied workspace ----------------------------------------------------------------------------------------------
_FRESH = {}


def _fresh_results(flags, jobs):
    if flags not in _FRESH:
        from zkp_amd.engine import Engine
        e = Engine(0)
        try:
            _FRESH[flags] = [_dev_call(e, *j[1:], flags) if j[0] == "dev" else e.msm_segments(j[1], j[2], j[4], j[3], flags) for j in jobs]
        finally:
            e.close()
    return _FRESH[flags]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("word", (0, 3, 0xFFFFFFFF), ids=lambda w: "fill%x" % w)
def test_classified_path_does_not_depend_on_what_the_workspace_held(G, word, flags):
    """the terms_only layout puts fin | A | B of the fold where the encoder's regions would start, and `part` of a class that skipped a term would keep
    what the workspace held: every word of it is 0, 3 or 0xFFFFFFFF before each call, and no call may grow it (a fresh allocation tests nothing)"""
    b_off, b_sc, b_pidx, b_points, flagged, _ = MC.mixed_job_with_invalid(G, TERMS_SPLIT + 1)
    n_own = TERMS_SPLIT + 65
    o_off, o_sc, o_rows, _ = MC.own_rows_job(n_own, seed=n_own)
    jobs = [("host", b_off, b_sc, b_pidx, b_points), ("dev", b_off, b_sc, b_pidx, b_points), ("host", o_off, o_sc, None, o_rows)]
    wants = [MC.expected("mixed-invalid", b_off, b_sc, b_pidx, b_points, flags)] * 2 + [MC.expected("own%d" % n_own, o_off, o_sc, None, o_rows, flags)]
    assert np.flatnonzero(wants[0][1]).tolist() == flagged
    fresh = _fresh_results(flags, jobs)
    e = _new_hooks()
    try:
        for (form, off, sc, pidx, points), (want, want_st), (f_out, f_st) in zip(jobs, wants, fresh):
            e.debug_fill_workspace(WS_FILL, word)
            size = e.debug_ws_bytes()
            assert size >= WS_FILL
            if form == "dev":
                got, st = _dev_call(e, off, sc, pidx, points, flags)
            else:
                got, st = e.msm_segments(off, sc, points, pidx, flags)
            kernels, sched = _seen(e)
            assert e.debug_ws_bytes() == size, "the call grew the workspace after the fill: raise WS_FILL"
            classified_and_folded(kernels, sched, flags)
            assert (st == want_st).all(), (form, np.flatnonzero(st != want_st)[:8])
            assert (got == want).all(), (form, np.flatnonzero((got != want).any(axis=1))[:8])
            assert (got == f_out).all() and (st == f_st).all(), "a fresh context computes other bytes"
    finally:
        e.close()


# ---- h. the 250,000-term rule of the throughput schedule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", (0, 1), ids=("below", "at"))
def test_single_use_points_take_the_ladder_from_250000_terms(hooks, eng, side):
    """constant time, _dev form, 16 segments: below kWideCallTerms terms single-use points get comb tables (comb_min 1), from there on the constant-time
    ladder (comb_min 2) and the grouped walk's size rule.  3 of 4 terms lie on 64 shared points, every 4th on a point of its own; every point is k B
    with a known k, so every segment's sum is (sum s_t k_t mod l) B exactly; the two short segments are also the oracle's"""
    from tests import test_gpu_thresholds as TH
    n_terms = WIDE_CALL - 1 + side
    rng = np.random.default_rng(n_terms)
    rest = n_terms - 45
    lens = [5] + [rest // 14] * 7 + [40] + [rest // 14] * 6 + [rest - 13 * (rest // 14)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    assert len(lens) == 16 and int(off[-1]) == n_terms
    pidx = rng.integers(0, 64, size=n_terms).astype(np.uint32)
    single = np.arange(0, n_terms, 4)
    pidx[single] = 64 + np.arange(len(single), dtype=np.uint32)
    sc = TH._rand_scalars(rng, n_terms)
    pts, logs = TH._points(eng, 64 + len(single))
    seen = {}
    out, st = _dev_call(hooks, off, sc, pidx, pts, ZKP_CT, probe=lambda e: seen.update(dev=_seen(e)))
    kernels, sched = seen["dev"]
    args = classified_and_folded(kernels, sched, ZKP_CT)
    assert sched.get("comb_min") == 1 + side and sched.get("grouped") == side, sched
    assert args[1:3] == ("4", "true" if side else "false") and kernels["tables"] == ["zkp::k_comb_tables_lane<4>"], kernels
    assert not st.any()
    for i in range(16):
        a, b = int(off[i]), int(off[i + 1])
        used, local = np.unique(pidx[a:b], return_inverse=True)
        assert bytes(out[i]) == TH._expected_point(TH._total_log(sc[a:b], local, [logs[u] for u in used])), i
        if b - a <= 40:
            exp, exp_st = C.msm_many(np.array([0, b - a], np.uint32), sc[a:b], local.astype(np.uint32), np.ascontiguousarray(pts[used]), 1)
            assert not exp_st.any() and (out[i] == exp[0]).all(), i


# ---- i. the example on an engine --------------------------------------------------------------------------------------------------------------------
def test_the_pedersen_vector_example_on_the_engine():
    """4 commitments over 1,100 generators: 4,404 constant-time terms on shared points, then two variable-time segments with a row per term (4 and
    1,101 terms)"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "pedersen_vector_batch.py"), "4", "1100"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "both sides agree" in r.stdout and "a wrong opening is rejected" in r.stdout

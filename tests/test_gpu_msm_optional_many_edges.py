"""zkp_msm_optional_many / _dev on the MI355X with CHOSEN scalars (tests/msm_optional_many_edge_cases.py): the bucket kernels in K-wide runs at
widths 7, 10 and 11 with buckets at every step of the part count, several huge buckets in one block of k_pip_bucket_merge, the digit-edge catalogue
in the slots of k_pip_prepare_csr's K-wide layout, the default merge form on both sides of its bucket count with skewed members, and the _dev
promises of include/zkp_mi355x.h (14): chunking over K, a member longer than max_seg, a max_seg that widens the window, a filled workspace.

tests/test_gpu_msm_optional_many.py checks the PLAN on evenly spread scalars; its fixtures are used here.  Every comparison is byte for byte and
status for status against the oracle's msm_many on the job itself; the notes of zkp_ctx_last_kernels must name the expected width and K of every
run.  The shipped engine gives the bytes; the test-hook engine forces the merge form (ZKP_TESTOPT_PIP_MERGE: 1 a quad per bucket, 2 a lane per
bucket), reports the form a call chose (zkp_debug_last_schedule) and fills the workspace (zkp_debug_fill_workspace).  What each job holds -- which
buckets, how many parts -- is asserted on the scalars in tests/test_host_msm_optional_many_edges.py."""
import numpy as np
import pytest

from tests import msm_optional_many_cases as OC
from tests import msm_optional_many_edge_cases as EC
from tests.test_gpu_msm_optional_many import S, _dev_job, _nothing_runs_after_a_gpu_error, _torch, call, check, eng, hooks      # noqa: F401 -- fixtures
from zkp_amd.engine import ZKP_TESTOPT_PIP_MERGE

pytestmark = pytest.mark.gpu
WS_FILL = 256 << 20                                      # many times what the largest filled case carves (three MSMs of 16,400 slots at c = 11)
WORDS = (0, 3, 0xFFFFFFFF)


def dev_job(e, off, sc, pidx, pts, max_seg):
    """_dev_job on copies (the helper module's arrays are read-only): torch buffers, the outputs poisoned"""
    return _dev_job(e, *(None if a is None else np.array(a) for a in (off, sc, pidx, pts)), max_seg)


def dev_run(e, d):
    d["enqueue"]()
    e.synchronize()
    return d["out"].cpu().numpy(), d["st"].cpu().numpy()


def forced_forms(hooks, off, sc, pidx, pts, want, want_st, c, name):
    """both merge forms on the test-hook engine: the bytes of the oracle, hence equal"""
    try:
        for mode in (1, 2):
            hooks.set_option(ZKP_TESTOPT_PIP_MERGE, mode)
            got, st = hooks.msm_optional_many(off, sc, pts, pidx)
            sched = hooks.last_schedule()
            assert sched.get("pip_c") == c and sched.get("pip_merge") == mode - 1, (name, mode, sched)
            assert (st == want_st).all() and (got == want).all(), (name, mode, np.flatnonzero((got != want).any(axis=1))[:8])
    finally:
        hooks.set_option(ZKP_TESTOPT_PIP_MERGE, 0)


def with_and_without_pidx(eng, hooks, name, job, c, K, n):
    off, sc, pidx, pts = job
    want, st, runs, _ = check(eng, name, off, sc, pidx, pts)
    assert runs == [(c, K, n, 0)], runs
    assert not st.any() and want.any(axis=1).all()
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    got, got_st, runs2, _ = call(eng, off, sc, None, rows)                # a point per term
    assert (got == want).all() and not got_st.any() and runs2 == runs
    forced_forms(hooks, off, sc, pidx, pts, want, st, c, name)
    forced_forms(hooks, off, sc, None, rows, want, st, c, name + " (a point per term)")
    return want, st


# ---- A. the digit-edge catalogue in the slots of a K-wide run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.WIDTHS)
def test_catalogue_values_in_the_slots_of_a_wide_run(eng, hooks, S, c):
    """six segments of one class.  At c = 7 the member of n // 2 + 1 = 151 terms is no longer than S and takes the term path in the same call: the run
    holds the other five, its shortest member (200 terms) a third padding"""
    lens = EC.catalogue_lens(c)
    K = sum(n > S for n in lens)
    assert K == (5 if c == 7 else 6)
    with_and_without_pidx(eng, hooks, "catalogue%d" % c, EC.catalogue_job(c)[:4], c, K, EC.LONGEST[c])
    if K < 6:
        assert eng.last_kernels().get("reduce"), eng.last_kernels()      # the term path


# ---- B. bucket sizes at every step of the part count --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.WIDTHS)
def test_bucket_size_ladder_in_a_wide_run(eng, hooks, c):
    off, sc, pidx, pts, lens, _ = EC.ladder_job(c)
    with_and_without_pidx(eng, hooks, "ladder%d" % c, (off, sc, pidx, pts), c, len(lens), max(lens))


# ---- C1. two buckets of more than kMergeSeqParts parts in one block of the merge -----------------------------------------------------------------------
@pytest.mark.parametrize("fold", (False, True), ids=("plain", "fold"))
def test_two_huge_buckets_in_one_merge_block(eng, hooks, fold):
    name = "twin-fold" if fold else "twin"
    off, sc, pidx, pts = EC.twin_huge_job(fold)
    want, st, runs, _ = check(eng, name, off, sc, pidx, pts)             # the default selection: a quad per bucket at 3 x 25,625 buckets
    assert runs == [(11, 3, max(EC.TWIN_LENS), 0)] and not st.any() and want.any(axis=1).all()
    got, got_st = hooks.msm_optional_many(off, sc, pts, pidx)
    sched = hooks.last_schedule()
    assert sched.get("pip_merge") == 0 and sched.get("pip_buckets") == 3 * EC.W1(11) * EC.B1(11), sched
    assert (got == want).all() and not got_st.any()
    forced_forms(hooks, off, sc, pidx, pts, want, st, 11, name)


def test_two_huge_buckets_in_a_single_segment(eng, hooks):
    off, sc, pidx, pts = EC.twin_single_job()
    want, st, runs, _ = check(eng, "twin-single", off, sc, pidx, pts)
    assert runs == [(11, 1, EC.TWIN_LENS[0], 0)] and not st.any() and want[0].any()
    assert (want[0] == OC.expected("twin", *EC.twin_huge_job())[0][0]).all()
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    assert eng.msm_optional(sc, rows) == bytes(want[0])                   # zkp_msm_optional: K = 1 through k_pip_prepare
    try:
        for mode in (1, 2):
            hooks.set_option(ZKP_TESTOPT_PIP_MERGE, mode)
            assert hooks.msm_optional(sc, rows) == bytes(want[0]), mode
            sched = hooks.last_schedule()
            assert sched.get("pip_c") == 11 and sched.get("pip_merge") == mode - 1, sched
    finally:
        hooks.set_option(ZKP_TESTOPT_PIP_MERGE, 0)
    forced_forms(hooks, off, sc, pidx, pts, want, st, 11, "twin-single")


@pytest.mark.parametrize("order", EC.TWIN_ORDERS, ids=lambda o: "".join(map(str, o)))
def test_two_huge_buckets_with_the_segments_in_every_order(eng, order):
    job = EC.twin_huge_job()
    want, want_st = OC.expected("twin", *job)
    off, sc, pidx, pts = EC.reordered(job, order)
    got, st, runs, _ = call(eng, off, sc, pidx, pts)
    assert runs == [(11, 3, max(EC.TWIN_LENS), 0)], runs                  # one class: one run, whatever the order
    assert not st.any() and (got == want[list(order)]).all(), np.flatnonzero((got != want[list(order)]).any(axis=1))


# ---- C2. the default merge form on both sides of its bucket count, skewed members first, in the middle and last ----------------------------------------
@pytest.mark.parametrize("side", (0, 1), ids=("below", "at"))
@pytest.mark.parametrize("c", EC.WIDTHS)
def test_default_merge_form_on_both_sides_of_the_rule(eng, hooks, S, c, side):
    width, K, seg = EC.threshold_cases(S)[2 * EC.WIDTHS.index(c) + side]
    assert width == c and K == {7: 212, 10: 37, 11: 20}[c] + side
    off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = EC.threshold_job(c, K, seg)
    want_d, st_d = OC.expected("threshold%d-%d" % (c, seg), off_d, sc_d, pidx_d, pts)
    assert not st_d.any() and len({bytes(r) for r in want_d}) == 4
    want = want_d[which]
    got, st, runs, _ = call(eng, off, sc, pidx, pts)
    assert runs == [(c, K, seg, 0)], runs
    assert not st.any() and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:8]
    got, st = hooks.msm_optional_many(off, sc, pts, pidx)
    sched = hooks.last_schedule()
    nb = K * EC.W1(c) * EC.B1(c)
    assert sched.get("pip_c") == c and sched.get("pip_buckets") == nb, sched
    assert sched.get("pip_merge") == int(nb >= EC.merge_lane_min_buckets()) == int(K in (213, 38, 21)), sched
    assert not st.any() and (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:8]


# ---- D. the _dev form -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    """{segments: (off, scalars, pidx, points, expected rows)} of the two chunked jobs: the oracle sums the distinct segments once for the tests below"""
    jobs = {}
    for n_seg, seg, distinct in EC.DEV_CHUNKS:
        off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = EC.dev_chunk_job(n_seg, seg, distinct)
        want_d, st_d = OC.expected("chunk%d" % n_seg, off_d, sc_d, pidx_d, pts)
        assert not st_d.any() and len({bytes(r) for r in want_d}) == distinct
        jobs[n_seg] = (off, sc, pidx, pts, want_d[which])
    return jobs


@pytest.mark.parametrize("n_seg,seg", [c[:2] for c in EC.DEV_CHUNKS], ids=lambda v: str(v))
def test_dev_form_more_segments_than_one_run_holds(eng, S, chunked, n_seg, seg):
    """chunked over K by the two limits (the run cap at 4,096 terms, the grid at S + 1): the second run starts at segment first + at of the job's own
    order.  Every row of the poisoned outputs is checked"""
    off, sc, pidx, pts, want = chunked[n_seg]
    out, st = dev_run(eng, dev_job(eng, off, sc, pidx, pts, seg))
    runs = OC.runs_of(eng.last_kernels().get("decode", []))
    assert runs == EC.dev_chunk_runs(n_seg, seg) and (seg == S + 1 or seg == 4096), runs
    assert not st.any() and (out == want).all(), np.flatnonzero((out != want).any(axis=1))[:8]


def test_dev_form_of_two_runs_recorded_once_and_replayed_twice(eng, chunked):
    torch = _torch()
    n_seg, seg, _ = EC.DEV_CHUNKS[0]
    off, sc, pidx, pts, want = chunked[n_seg]
    d = dev_job(eng, off, sc, pidx, pts, seg)
    out, st = dev_run(eng, d)                                             # outside the capture first: the workspace has its size
    assert len(OC.runs_of(eng.last_kernels().get("decode", []))) == 2 and not st.any() and (out == want).all()
    for t in (d["out"], d["st"]):
        t.fill_(0xCD)
    torch.cuda.synchronize()
    with eng.capture() as cap:
        d["enqueue"]()
    assert bool((d["out"] == 0xCD).all().item())                          # recorded, not run
    try:
        for _ in range(2):
            cap.graph.launch()
            eng.synchronize()
            assert (d["out"].cpu().numpy() == want).all() and not d["st"].cpu().numpy().any()
            for t in (d["out"], d["st"]):
                t.fill_(0xCD)
            torch.cuda.synchronize()
    finally:
        cap.graph.close()


def test_dev_form_with_a_segment_longer_than_max_seg(eng):
    """that segment's own row is unspecified, the other rows are right: the lanes of a run number max_seg per MSM (k_pip_prepare_csr), so the long
    member is read up to max_seg terms and nothing of it reaches a neighbour"""
    off, sc, pidx, pts = EC.dev_long_member_job()
    want, want_st = OC.expected("dev-long", off, sc, pidx, pts)
    keep = [i for i in range(len(off) - 1) if i != EC.DEV_LONG_SEG]
    assert not want_st.any() and want[keep].any(axis=1).all()
    out, st = dev_run(eng, dev_job(eng, off, sc, pidx, pts, EC.DEV_LONG_MAX_SEG))
    assert OC.runs_of(eng.last_kernels().get("decode", [])) == [(7, len(off) - 1, EC.DEV_LONG_MAX_SEG, 0)]
    assert (out[keep] == want[keep]).all() and (st[keep] == want_st[keep]).all()


@pytest.mark.parametrize("max_seg,c", ((4096, 10), (8192, 11)))
def test_dev_form_max_seg_widens_the_window(eng, max_seg, c):
    """the ladder job of width 7 padded to the first run length of widths 10 and 11: the same sums through other windows"""
    off, sc, pidx, pts, lens, _ = EC.ladder_job(7)
    assert EC.pick_c(max(lens)) == 7
    want, want_st = OC.expected("ladder7", off, sc, pidx, pts)
    host, host_st, host_runs, _ = call(eng, off, sc, pidx, pts)
    assert host_runs == [(7, len(lens), max(lens), 0)]
    out, st = dev_run(eng, dev_job(eng, off, sc, pidx, pts, max_seg))
    assert OC.runs_of(eng.last_kernels().get("decode", [])) == [(c, len(lens), max_seg, 0)]
    assert (out == host).all() and (st == host_st).all() and (out == want).all() and (st == want_st).all()


def _filled(hooks, word):
    hooks.debug_fill_workspace(WS_FILL, word)
    size = hooks.debug_ws_bytes()
    assert size >= WS_FILL
    return size


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
def test_results_do_not_depend_on_what_the_workspace_held(hooks, S, word):
    """every word of the workspace is 0, 3 or 0xFFFFFFFF in front of the _dev run path (one class padded to max_seg: not its host-pointer form's plan), of
    the _dev term path (generic bounds, a device-written index) and of the host form on a ladder job; no call may grow the workspace after the fill"""
    # the _dev run path: the twin job padded to twice its longest segment
    off, sc, pidx, pts = EC.twin_huge_job()
    want, want_st = OC.expected("twin", off, sc, pidx, pts)
    max_seg = 2 * max(EC.TWIN_LENS)
    d = dev_job(hooks, off, sc, pidx, pts, max_seg)
    size = _filled(hooks, word)
    out, st = dev_run(hooks, d)
    sched = hooks.last_schedule()
    assert hooks.debug_ws_bytes() == size, "the call grew the workspace after the fill: raise WS_FILL"
    assert sched.get("pip_c") == 11 and sched.get("pip_buckets") == 3 * EC.W1(11) * EC.B1(11), sched
    assert (out == want).all() and (st == want_st).all(), np.flatnonzero((out != want).any(axis=1))
    # the _dev term path: max_seg = S, a point per term
    off, sc, pidx, pts = EC.dev_term_path_job(S)
    want, want_st = OC.expected("dev-terms", off, sc, pidx, pts)
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    d = dev_job(hooks, off, sc, None, rows, S)
    size = _filled(hooks, word)
    out, st = dev_run(hooks, d)
    sched = hooks.last_schedule()
    assert hooks.debug_ws_bytes() == size
    assert "pip_c" not in sched, sched
    assert (out == want).all() and (st == want_st).all(), np.flatnonzero((out != want).any(axis=1))
    # the host form on the ladder job of width 10
    off, sc, pidx, pts, lens, _ = EC.ladder_job(10)
    want, want_st = OC.expected("ladder10", off, sc, pidx, pts)
    size = _filled(hooks, word)
    out, st = hooks.msm_optional_many(off, sc, pts, pidx)
    sched = hooks.last_schedule()
    assert hooks.debug_ws_bytes() == size
    assert sched.get("pip_c") == 10 and sched.get("pip_buckets") == len(lens) * EC.W1(10) * EC.B1(10), sched
    assert (out == want).all() and (st == want_st).all(), np.flatnonzero((out != want).any(axis=1))

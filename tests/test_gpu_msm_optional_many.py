"""Many variable-time multiscalar sums with long segments on the MI355X: zkp_msm_optional_many / _dev run zkp_msm_optional's bucket kernels on K
segments side by side (k_pip_prepare_csr, k_pip_tile_hist .. k_pip_combine, k_pip_rows), segments of at most S = zkp_msm_optional_many_min_segment()
terms on the term path, with the toolbox routing in front.  Every comparison is byte for byte and status for status against the oracle's msm_many
on the same job (tests/msm_optional_many_cases.py); single segments and equal segments also against zkp_msm_optional on the same operands.  The plan
-- which segments share a run, how wide it is -- is read from the kernel notes of zkp_ctx_last_kernels, never from a copy of the size rules: the
rules' constants (the run cap, the window widths' W1) are read from the sources."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import cbind as C
from tests import msm_optional_many_cases as OC
from tests import msm_segments_cases as MC
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_VARTIME

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 0xFFFFFFFF


def W1(c):
    """pip_cfg<C>::W1: the windows of a run of width c, the carry window included"""
    return (256 + c - 1) // c + 1


def run_cap():
    src = open(os.path.join(ROOT, "zkp_amd", "csrc", "pip_segments.h")).read()
    m = re.search(r"constexpr uint64_t kPipRunCapTerms = 1u << (\d+);", src)
    assert m
    return 1 << int(m.group(1))


@pytest.fixture(scope="module")
def eng():
    """the shipped library with profiling on: the kernel notes are the plan"""
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    e.set_profiling(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def S(eng):
    s = int(eng._lib.zkp_msm_optional_many_min_segment())
    assert s == MC.threshold("kSmallOptional")
    return s


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(eng):
    """a call that faulted leaves the device in error for every context of the process: the session ends there instead of launching the remaining
    cases on that card"""
    yield
    try:
        eng.synchronize()
    except Exception as e:                                   # noqa: BLE001 -- whatever the runtime reports
        pytest.exit("the shared context reports a GPU error; nothing further is started: %s" % e, returncode=3)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def call(e, off, sc, pidx, points):
    """-> (out, status, runs named by the notes, all decode-kind notes)"""
    got, st = e.msm_optional_many(off, sc, points, pidx)
    names = e.last_kernels()
    return got, st, OC.runs_of(names.get("decode", [])), names


def check(e, name, off, sc, pidx, points):
    want, want_st = OC.expected(name, off, sc, pidx, points)
    got, st, runs, names = call(e, off, sc, pidx, points)
    assert (st == want_st).all(), name
    assert (got == want).all(), name
    return want, want_st, runs, names


# ---- 1. single segments: both sides of the term-path rule and of pick_c's 7 | 10 and 10 | 11 boundaries ----------------------------------------
@pytest.mark.parametrize("which", range(7))
def test_single_segments(eng, S, which):
    n = OC.single_lengths(S)[which]
    off, sc, pidx, pts = OC.job([n], seed=n)
    want, st, runs, names = check(eng, "single%d" % n, off, sc, pidx, pts)
    assert not st.any() and want[0].any()
    if n <= S:
        assert runs == [] and names.get("reduce"), names                 # the term path
    else:
        assert runs == [(7 if n < 4096 else 10 if n < 8192 else 11, 1, n, 0)], runs
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    one = eng.msm_optional(sc, rows)
    assert one == bytes(want[0])
    got, got_st = eng.msm_optional_many(off, sc, rows, None)
    assert (got == want).all() and not got_st.any()


# ---- 2. the ragged job, classes interleaved ----------------------------------------------------------------------------------------------------
def test_ragged_job_plan_and_bytes(eng, S):
    lens = OC.shuffled(OC.ragged_lengths(S), seed=3)
    off, sc, pidx, pts = OC.job(lens, seed=2)
    srt = sorted(n for n in lens if n > S)
    pos = [srt.index(n) for n in lens if n > S]
    assert any(abs(a - b) > 1 for a, b in zip(pos, pos[1:]))            # neighbours in the job are not neighbours in length: the classes interleave
    want, st, runs, names = check(eng, "ragged", off, sc, pidx, pts)
    assert not st.any() and not want[np.diff(off.astype(np.int64)) == 0].any()
    members = OC.check_plan(runs, lens, S)                                # no run pads a member by a factor of two or more
    assert names.get("reduce"), names                                     # the segments of 1, 2 and S terms: the term path, in the same call
    # the class rule (2 * len > the class's longest): 513 joins the class of 1,025, 512 does not
    assert any(1025 in m and 1024 in m and 513 in m for m in members), members
    assert not any(1025 in m and 512 in m for m in members) and any(512 in m and 511 in m and 300 in m for m in members), members
    assert any(m == [8199, 5000] for m in members) and [4096] in members and [S + 1] in members, members
    # a point per term
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    got, got_st, runs2, _ = call(eng, off, sc, None, rows)
    assert (got == want).all() and (got_st == st).all() and runs2 == runs


# ---- 3. invalid encodings ------------------------------------------------------------------------------------------------------------------------
def test_invalid_encodings_flag_exactly_the_referencing_segments(eng, S):
    off, sc, pidx, points, flagged, lens = OC.with_invalid(S)
    want, st, runs, names = check(eng, "invalid", off, sc, pidx, points)
    assert np.flatnonzero(st).tolist() == flagged and not want[flagged].any()
    members = OC.check_plan(runs, lens, S)
    assert members[0][0] == 1300 and 700 in members[0] and any(600 in m and 3 * S in m for m in members[1:]), members   # one bad row, two classes
    clean_off, clean_sc, clean_pidx, pts = OC.job(lens, seed=5)
    clean, _ = OC.expected("invalid-clean", clean_off, clean_sc, clean_pidx, pts)
    rest = [i for i in range(len(lens)) if i not in flagged]
    assert (want[rest] == clean[rest]).all() and want[[1, 4, 9]].any(axis=1).all()    # the run neighbour (3 S terms) and the short ones are untouched


# ---- 4. identity results in long form ------------------------------------------------------------------------------------------------------------
def test_identity_results(eng, S):
    off, sc, pidx, pts, identity, others = OC.identity_cases(S)
    want, st, runs, _ = check(eng, "identity", off, sc, pidx, pts)
    assert sum(r[1] for r in runs) == len(off) - 1                        # every segment is longer than S: all of them in runs
    assert not st.any() and not want[identity].any() and want[others].any(axis=1).all()


# ---- 5. chunking over K: more segments of S + 1 terms than grid.y holds at c = 7 -----------------------------------------------------------------
def test_more_segments_than_one_run_holds(eng, S):
    k_grid = 65535 // W1(7)
    n_seg = k_grid + 1
    assert (S + 1) * n_seg < run_cap()                                    # it is the grid that cuts here, not the cap
    off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = OC.repeated_job(n_seg, S + 1, 41, seed=8)
    want_d, st_d = OC.expected("chunk-distinct", off_d, sc_d, pidx_d, pts)
    assert not st_d.any() and len({bytes(r) for r in want_d}) == 41
    got, st, runs, _ = call(eng, off, sc, pidx, pts)
    assert runs == [(7, k_grid, S + 1, 0), (7, 1, S + 1, k_grid)], runs
    assert not st.any() and (got == want_d[which]).all()


# ---- 6. the run cap: equal segments, just at and just above it -----------------------------------------------------------------------------------
@pytest.mark.parametrize("over", (0, 1))
def test_run_cap(eng, S, over):
    seg = 4096
    k_cap = run_cap() // seg
    assert k_cap < 65535 // W1(10)
    n_seg = k_cap + over
    off, sc, pidx, pts, which, (off_d, sc_d, pidx_d) = OC.repeated_job(n_seg, seg, 7, seed=9)
    want_d, st_d = OC.expected("cap-distinct", off_d, sc_d, pidx_d, pts)
    got, st, runs, _ = call(eng, off, sc, pidx, pts)
    assert runs == ([(10, k_cap, seg, 0), (10, 1, seg, k_cap)] if over else [(10, k_cap, seg, 0)]), runs
    assert not st.any() and not st_d.any() and (got == want_d[which]).all()


# ---- 7. the _dev form ------------------------------------------------------------------------------------------------------------------------------
def _dev_job(e, off, sc, pidx, pts, max_seg, fill=0xAB):
    torch = _torch()
    dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
    n_seg, n_terms = len(off) - 1, int(off[-1])
    d = dict(off=dev(off), sc=dev(sc), pidx=None if pidx is None else dev(pidx), pts=dev(pts),
             out=torch.full((n_seg, 32), fill, dtype=torch.uint8, device="cuda:0"), st=torch.full((n_seg,), fill, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    d["enqueue"] = lambda: e.msm_optional_many_dev(n_seg, d["off"].data_ptr(), d["sc"].data_ptr(), None if pidx is None else d["pidx"].data_ptr(),
                                                   d["pts"].data_ptr(), len(pts), n_terms, max_seg, d["out"].data_ptr(), d["st"].data_ptr())
    return d


def test_dev_form_one_class_whatever_max_seg(eng, S):
    lens = [200, 400, 333, 250, 399]
    off, sc, pidx, pts = OC.job(lens, seed=12)
    want, want_st = OC.expected("dev5", off, sc, pidx, pts)
    for max_seg in (400, 1000):
        d = _dev_job(eng, off, sc, pidx, pts, max_seg)
        d["enqueue"]()
        eng.synchronize()
        runs = OC.runs_of(eng.last_kernels().get("decode", []))
        assert runs == [(7, 5, max_seg, 0)], runs
        assert (d["out"].cpu().numpy() == want).all() and (d["st"].cpu().numpy() == want_st).all(), max_seg
    # a point per term, and an index out of range: its segment is flagged, every other row is right
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    d = _dev_job(eng, off, sc, None, rows, 400)
    d["enqueue"]()
    eng.synchronize()
    assert (d["out"].cpu().numpy() == want).all() and (d["st"].cpu().numpy() == want_st).all()
    bad = MC.invalid_rows()[:1]
    wild = pidx.copy()
    wild[int(off[2]) + 7] = len(pts) + 1000                               # clamped to the last row, which does not decode
    d = _dev_job(eng, off, sc, wild, np.concatenate([pts, bad]), 400)
    d["enqueue"]()
    eng.synchronize()
    st = d["st"].cpu().numpy()
    assert st.tolist() == [0, 0, 1, 0, 0] and not d["out"].cpu().numpy()[2].any()
    assert (np.delete(d["out"].cpu().numpy(), 2, axis=0) == np.delete(want, 2, axis=0)).all()


def test_dev_form_takes_the_term_path_up_to_S(eng, S):
    lens = [S, 5, 0, 100, S - 1]
    off, sc, pidx, pts = OC.job(lens, seed=13)
    want, want_st = OC.expected("devS", off, sc, pidx, pts)
    d = _dev_job(eng, off, sc, pidx, pts, S)
    d["enqueue"]()
    eng.synchronize()
    names = eng.last_kernels()
    assert OC.runs_of(names.get("decode", [])) == [] and names.get("reduce"), names
    assert (d["out"].cpu().numpy() == want).all() and (d["st"].cpu().numpy() == want_st).all()
    d = _dev_job(eng, off, sc, pidx, pts, S + 1)                          # the other side of the rule: one run
    d["enqueue"]()
    eng.synchronize()
    assert OC.runs_of(eng.last_kernels().get("decode", [])) == [(7, 5, S + 1, 0)]
    assert (d["out"].cpu().numpy() == want).all() and (d["st"].cpu().numpy() == want_st).all()
    # every segment empty
    d = _dev_job(eng, np.zeros(4, np.uint32), sc[:0], None, pts[:0], 500)
    d["enqueue"]()
    eng.synchronize()
    assert not d["out"].cpu().numpy().any() and not d["st"].cpu().numpy().any()


def test_dev_form_recorded_once_and_replayed_twice(eng, S):
    torch = _torch()
    lens = [200, 400, 333, 250, 399]
    off, sc, pidx, pts = OC.job(lens, seed=12)
    want, want_st = OC.expected("dev5", off, sc, pidx, pts)
    d = _dev_job(eng, off, sc, pidx, pts, 400)
    d["enqueue"]()                                                        # outside the capture first: the workspace has its size
    eng.synchronize()
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
            assert (d["out"].cpu().numpy() == want).all() and (d["st"].cpu().numpy() == want_st).all()
            for t in (d["out"], d["st"]):
                t.fill_(0xCD)
            torch.cuda.synchronize()
    finally:
        cap.graph.close()


# ---- 8. c = 16: one segment of 2^21 terms over the catalogue, and a short neighbour ------------------------------------------------------------
def test_two_to_the_21_terms_on_shared_points(eng, S):
    big, small = 1 << 21, 300
    cat = MC.catalogue()
    rng = np.random.default_rng(21)
    sc = rng.integers(0, 256, size=(big + small, 32), dtype=np.uint8)
    sc[:4] = OC.PC.rows([0, OC.L, 2 ** 256 - 1, OC.L - 1])
    pidx = rng.integers(0, len(cat), size=big + small).astype(np.uint32)
    off = np.array([0, big, big + small], np.uint32)
    # per-row sums of the scalars mod l in Python integers: 32-bit limbs summed per row in uint64 (2^21 x 2^32 < 2^64), then recombined
    order = np.argsort(pidx[:big], kind="stable")
    starts = np.searchsorted(pidx[:big][order], np.arange(len(cat)))
    limbs = np.add.reduceat(sc[:big].view("<u4")[order].astype(np.uint64), starts, axis=0)
    sums = [sum(int(limbs[r, k]) << (32 * k) for k in range(8)) % OC.L for r in range(len(cat))]
    assert np.bincount(pidx[:big], minlength=len(cat)).min() > 0         # (reduceat needs every row used)
    want_big, st_big = C.msm_many(np.array([0, len(cat)], np.uint32), OC.PC.rows(sums), np.arange(len(cat), dtype=np.uint32), cat, ZKP_VARTIME)
    want_small, st_small = C.msm_many(np.array([0, small], np.uint32), sc[big:], pidx[big:], cat, ZKP_VARTIME)
    got, st, runs, _ = call(eng, off, sc, pidx, cat)
    assert runs == [(16, 1, big, 0), (7, 1, small, 1)], runs
    assert not st.any() and not st_big.any() and not st_small.any()
    assert (got[0] == want_big[0]).all() and (got[1] == want_small[0]).all() and got[0].any()


# ---- 9. the workspace: what earlier calls left there changes nothing --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(S):
    lens = OC.shuffled(OC.ragged_lengths(S), seed=3)
    off, sc, pidx, pts = OC.job(lens, seed=2)
    return (off, sc, pidx, pts) + OC.expected("ragged", off, sc, pidx, pts)


@pytest.fixture(scope="module")
def hooks():
    from zkp_amd.engine import Engine
    e = Engine(0, test_hooks=True)
    yield e
    e.close()


@pytest.mark.parametrize("word", (0, 3, 0xFFFFFFFF), ids=lambda w: "fill%x" % w)
def test_results_do_not_depend_on_what_the_workspace_held(hooks, eng, ragged, word):
    off, sc, pidx, pts, want, want_st = ragged
    fresh, fresh_st = eng.msm_optional_many(off, sc, pts, pidx)          # (the shared context: its workspace is whatever the cases before left)
    hooks.debug_fill_workspace(256 << 20, word)
    size = hooks.debug_ws_bytes()
    got, st = hooks.msm_optional_many(off, sc, pts, pidx)
    assert hooks.debug_ws_bytes() == size                                 # the call ran inside the filled workspace
    assert (got == want).all() and (st == want_st).all() and (got == fresh).all() and (st == fresh_st).all()


def test_results_behind_a_cmz_prove_and_batch_verify_on_the_same_context(ragged):
    from tests import test_gpu_workspace_residue as WR
    from zkp_amd.engine import Engine
    off, sc, pidx, pts, want, want_st = ragged
    n = 264
    es, e = Engine(0), Engine(0)
    try:
        fresh, fresh_st = e.msm_optional_many(off, sc, pts, pidx)        # a fresh context
        b = WR._batch(es, "cmz", n)
        chal, resp, coms, _ = WR._prove_dev(e, b["fst"], n, b["ts0"], b["pos"], b["secrets"], b["table"], b["entropy"], b["m"], b["nc"])
        assert (coms == b["coms"]).all()
        w = np.random.default_rng(n + 3).integers(0, 256, size=(b["nc"], n, 16), dtype=np.uint8)
        out, bst, _ = WR._batch_verify(e, b, 1, n, resp, coms, w)
        assert not out.any() and not bst.any()                            # the batch verifies
        got, st = e.msm_optional_many(off, sc, pts, pidx)
        assert (got == want).all() and (st == want_st).all() and (got == fresh).all() and (st == fresh_st).all()
    finally:
        e.close()
        es.close()


def test_timing_total_spans_a_call_of_more_runs_than_timing_marks(hooks):
    """zkp_ctx_last_timing keeps 32 marks and a run records four: a call of 16 runs must still report the time of all 16.  Runs follow each other on one
    stream, so 16 equal runs take about four times as long as the first 4 of them; a total cut off at the mark limit would say 7.75 / 4 = 1.9 times."""
    from zkp_amd.engine import ZKP_TESTOPT_PIP_RUN_CAP
    seg = 4096
    off, sc, pidx, pts, which, _ = OC.repeated_job(16, seg, 4, seed=15)
    hooks.set_option(ZKP_TESTOPT_PIP_RUN_CAP, seg)
    hooks.set_profiling(True)
    try:
        def total(n_seg):
            best = None
            for _ in range(4):
                hooks.msm_optional_many(off[:n_seg + 1], sc[:n_seg * seg], pts, pidx[:n_seg * seg])
                kinds, t = hooks.last_timing()
                assert len(OC.runs_of(hooks.last_kernels().get("decode", []))) == n_seg
                assert abs(sum(kinds.values()) - t) <= 0.01 * t           # the per-kind split still adds up to the total
                best = t if best is None else min(best, t)
            return best
        t4, t16 = total(4), total(16)
        print("4 runs %.3f ms, 16 runs %.3f ms" % (t4, t16))
        assert t16 > 3.0 * t4, (t4, t16)
    finally:
        hooks.set_profiling(False)
        hooks.set_option(ZKP_TESTOPT_PIP_RUN_CAP, 0)


# ---- 10. toolbox routing ----------------------------------------------------------------------------------------------------------------------------
def test_toolbox_routes_on_both_sides_of_the_bucket_threshold(eng, S):
    old = T.get_msm_bucket_min_segment()
    try:
        T.set_msm_bucket_min_segment(1024)
        for longest in (1023, 1024):
            off, sc, pidx, pts = OC.job([300, longest, 5], seed=longest)
            want, want_st = OC.expected("route%d" % longest, off, sc, pidx, pts)
            got, st = T.optional_multiscalar_mul(eng, off, sc, pts, pidx)
            names = eng.last_kernels()
            runs = OC.runs_of(names.get("decode", []))
            assert (got == want).all() and (st == want_st).all()
            if longest < 1024:
                reduce = ";".join(names.get("reduce", []))                  # zkp_msm_many: one lane per MSM, or the shared-inversion encoder
                assert runs == [] and names.get("terms") and ("k_reduce_encode" in reduce or "k_encode_prepare" in reduce), names
                assert "k_pip_prepare" not in ";".join(names.get("decode", [])) and "k_sum_fold" not in reduce, names
            else:
                assert [r[1:3] for r in runs] == [(1, 1024), (1, 300)], names
        # "never": everything on the route zkp_multiscalar_sum_batch gives it
        T.set_msm_bucket_min_segment(NEVER)
        off, sc, pidx, pts = OC.job([300, 1024, 5], seed=1024)
        got, st = T.optional_multiscalar_mul(eng, off, sc, pts, pidx)
        names = eng.last_kernels()
        assert OC.runs_of(names.get("decode", [])) == [] and "k_sum_fold" in ";".join(names.get("reduce", [])), names      # zkp_msm_segments
        want, want_st = OC.expected("route1024", off, sc, pidx, pts)
        assert (got == want).all() and (st == want_st).all()
        # 0: always the bucket method (segments up to S still take the term path inside the call)
        T.set_msm_bucket_min_segment(0)
        got, st = T.optional_multiscalar_mul(eng, off, sc, pts, pidx)
        assert len(OC.runs_of(eng.last_kernels().get("decode", []))) == 2 and (got == want).all()
    finally:
        T.set_msm_bucket_min_segment(old)


# ---- 11. K equal segments against K calls of zkp_msm_optional ---------------------------------------------------------------------------------------
def test_equal_segments_against_one_call_each(eng, S):
    K, n = 9, 700
    off, sc, pidx, pts = OC.job([n] * K, seed=14)
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    got, st, runs, _ = call(eng, off, sc, None, rows)
    assert runs == [(7, K, n, 0)] and not st.any()
    for k in range(K):
        assert eng.msm_optional(sc[k * n:(k + 1) * n], rows[k * n:(k + 1) * n]) == bytes(got[k]), k
    want, _ = OC.expected("equal", off, sc, pidx, pts)
    assert (got == want).all()


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    off, sc, pidx, pts = OC.job([3, 0, 5], seed=4)
    out, st = np.full((3, 32), 0xEE, np.uint8), np.full(3, 0xEE, np.uint8)
    OF, SCp, PI, P, O, ST = (a.ctypes.data for a in (off, sc, pidx, pts, out, st))
    f = lib.zkp_msm_optional_many
    assert f(h, 0, None, None, None, None, 0, None, None) == 0
    assert f(h, 3, np.array([1, 3, 3, 8], np.uint32).ctypes.data, SCp, PI, P, len(pts), O, ST) == -2
    assert f(h, 3, np.array([0, 5, 3, 8], np.uint32).ctypes.data, SCp, PI, P, len(pts), O, ST) == -2
    assert f(h, 3, OF, SCp, PI, P, int(pidx.max()), O, ST) == -2
    assert f(h, 3, OF, SCp, None, P, len(pts), O, ST) == -2
    for args in ((None, SCp, PI, P), (OF, None, PI, P), (OF, SCp, PI, None)):
        assert f(h, 3, *args, len(pts), O, ST) == -2
    assert f(h, 3, OF, SCp, PI, P, len(pts), None, ST) == -2 and f(h, 3, OF, SCp, PI, P, len(pts), O, None) == -2
    assert (out == 0xEE).all() and (st == 0xEE).all()
    got, gst = eng.msm_optional_many(off, sc, pts, pidx)
    want, want_st = OC.expected("args", off, sc, pidx, pts)
    assert (got == want).all() and (gst == want_st).all()


def test_the_contest_tallies_example_on_the_engine():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "contest_tallies_batch.py"), "6", "700"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "agree" in r.stdout

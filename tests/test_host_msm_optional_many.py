"""Many variable-time multiscalar sums with long segments on the host backend (no GPU): toolbox.optional_multiscalar_mul with eng = None is the CSR MSM
behind zkp_multiscalar_sum_batch with ZKP_VARTIME (the host has no bucket method).  Byte for byte and status for status against the oracle's
msm_many on the same job (tests/msm_optional_many_cases.py): the ragged job with and without pidx, invalid encodings, the identity cases, the
argument errors; then what a CPU can say about the surface -- the declarations, the threshold's setter, the segment rule's constant."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import msm_optional_many_cases as OC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (1, 5)
BAD_STATEMENT = -10
NEVER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def S():
    from zkp_amd.engine import load_library
    s = int(load_library().zkp_msm_optional_many_min_segment())            # pure arithmetic: no context, no GPU
    from tests import size_thresholds as ST
    assert {r["value"] for r in ST.ROWS if r["const"] == "kSmallOptional"} == {s}
    return s


def check(name, off, sc, pidx, points, threads=THREADS):
    want, want_st = OC.expected(name, off, sc, pidx, points)
    for t in threads:
        got, st = T.optional_multiscalar_mul(None, off, sc, points, pidx, threads=t)
        assert (st == want_st).all(), (name, t)
        assert (got == want).all(), (name, t)
    return want, want_st


def test_ragged_job_with_shuffled_classes(S):
    lens = OC.shuffled(OC.ragged_lengths(S), seed=3)
    assert sorted(lens) == sorted(OC.ragged_lengths(S)) and lens != OC.ragged_lengths(S)
    off, sc, pidx, pts = OC.job(lens, seed=2)
    assert len(pts) == 512
    want, st = check("ragged", off, sc, pidx, pts)
    empty = np.flatnonzero(np.diff(off.astype(np.int64)) == 0)
    assert len(empty) == 3 and not want[empty].any() and not st.any()
    # the same bytes as the call with a flags argument, and with a point per term
    old, old_st = T.multiscalar_sum(None, off, sc, pts, pidx, OC.VARTIME)
    assert (old == want).all() and (old_st == st).all()
    _, _, rows = OC.own_points(off, sc, pidx, pts)
    got, got_st = T.optional_multiscalar_mul(None, off, sc, rows, None, threads=5)
    assert (got == want).all() and (got_st == st).all()
    with pytest.raises(Exception):
        T.optional_multiscalar_mul(None, off, sc, rows[:-1], None)         # n_points != n_terms


def test_invalid_encodings_flag_their_segments_and_no_other(S):
    off, sc, pidx, points, flagged, lens = OC.with_invalid(S)
    want, st = check("invalid", off, sc, pidx, points)
    assert np.flatnonzero(st).tolist() == flagged and not want[flagged].any()
    clean_off, clean_sc, clean_pidx, pts = OC.job(lens, seed=5)
    clean, _ = OC.expected("invalid-clean", clean_off, clean_sc, clean_pidx, pts)
    rest = [i for i in range(len(lens)) if i not in flagged]
    assert (want[rest] == clean[rest]).all() and want[[1, 4, 9]].any(axis=1).all()


def test_identity_results(S):
    off, sc, pidx, pts, identity, others = OC.identity_cases(S)
    want, st = check("identity", off, sc, pidx, pts)
    assert not st.any() and not want[identity].any() and want[others].any(axis=1).all()


def test_argument_errors_write_nothing():
    off, sc, pidx, pts = OC.job([3, 0, 5], seed=4)
    out, st = np.full((3, 32), 0xEE, np.uint8), np.full(3, 0xEE, np.uint8)
    OF, SCp, PI, P, O, ST = (a.ctypes.data for a in (off, sc, pidx, pts, out, st))
    call = T.lib().zkp_multiscalar_optional_batch
    assert call(None, 0, None, None, None, None, 0, 0, None, None) == 0
    one = np.array([1, 3, 3, 8], np.uint32)
    assert call(None, 3, one.ctypes.data, SCp, PI, P, len(pts), 0, O, ST) == BAD_STATEMENT     # off[0] != 0
    dec = np.array([0, 5, 3, 8], np.uint32)
    assert call(None, 3, dec.ctypes.data, SCp, PI, P, len(pts), 0, O, ST) == BAD_STATEMENT     # decreasing
    assert call(None, 3, OF, SCp, PI, P, int(pidx.max()), 0, O, ST) == BAD_STATEMENT           # an index out of range
    assert call(None, 3, OF, SCp, None, P, len(pts), 0, O, ST) == BAD_STATEMENT                # no pidx: n_points must be the number of terms
    for args in ((None, SCp, PI, P), (OF, None, PI, P), (OF, SCp, PI, None)):
        assert call(None, 3, *args, len(pts), 0, O, ST) == BAD_STATEMENT
    assert call(None, 3, OF, SCp, PI, P, 0, 0, O, ST) == BAD_STATEMENT                         # terms without points
    assert call(None, 3, OF, SCp, PI, P, len(pts), 0, None, ST) == BAD_STATEMENT
    assert call(None, 3, OF, SCp, PI, P, len(pts), 0, O, None) == BAD_STATEMENT
    assert (out == 0xEE).all() and (st == 0xEE).all()
    # the device entry points refuse a NULL context themselves
    from zkp_amd.engine import load_library
    hip = load_library()
    assert hip.zkp_msm_optional_many(None, 3, OF, SCp, PI, P, len(pts), O, ST) == -2
    assert hip.zkp_msm_optional_many_dev(None, 3, OF, SCp, PI, P, len(pts), 8, 5, O, ST) == -2
    assert (out == 0xEE).all() and (st == 0xEE).all()


def test_declarations_threshold_setter_and_rust_agree(S):
    from zkp_amd import cabi
    tb, dev = cabi.signatures("zkp_toolbox.h"), cabi.signatures("zkp_mi355x.h")
    assert {"zkp_multiscalar_optional_batch", "zkp_toolbox_set_msm_bucket_min_segment", "zkp_toolbox_get_msm_bucket_min_segment"} <= set(tb)
    assert {"zkp_msm_optional_many", "zkp_msm_optional_many_dev", "zkp_msm_optional_many_min_segment"} <= set(dev)
    rust = open(os.path.join(ROOT, "rust", "zkp-mi355x-sys", "src", "lib.rs")).read()
    for name in ("zkp_msm_optional_many", "zkp_msm_optional_many_dev", "zkp_msm_optional_many_min_segment", "zkp_multiscalar_optional_batch"):
        assert "pub fn %s(" % name in rust
    old = T.get_msm_bucket_min_segment()
    assert old > S                                                # runs exist above S only; NEVER is a legal default
    try:
        T.set_msm_bucket_min_segment(77)
        assert T.get_msm_bucket_min_segment() == 77
        T.set_msm_bucket_min_segment(NEVER)
        assert T.get_msm_bucket_min_segment() == NEVER
    finally:
        T.set_msm_bucket_min_segment(old)


def test_plan_reader_accepts_a_sound_plan_and_refuses_padding_by_two(S):
    """the helper the GPU tests read the kernel notes with, on notes written by hand"""
    names = ["k_pip_prepare_csr<7>@K=2,n=1024,at=0", "k_pip_prepare_csr<7>@K=1,n=300,at=2", "k_terms_r4"]
    runs = OC.runs_of(names)
    assert runs == [(7, 2, 1024, 0), (7, 1, 300, 2)]
    assert OC.check_plan(runs, [0, 5, 1024, 513, 300, S], S) == [[1024, 513], [300]]
    with pytest.raises(AssertionError):
        OC.check_plan(runs, [1024, 512, 300], S)                 # 512 in a run of 1,024 slots: padded by two
    with pytest.raises(AssertionError):
        OC.check_plan(runs[:1], [1024, 513, 300], S)             # a long segment no run holds


def test_the_contest_tallies_example_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "contest_tallies_batch.py"), "3", "40", "--host"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "agree" in r.stdout

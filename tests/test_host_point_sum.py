"""Batched RistrettoPoint sums on the host backend (ctx == NULL): zkp_point_add_batch and zkp_point_sum_batch run hostbk::add_points_n /
sum_points_n -- the kernels' point formulas over the host field -- on the host threads.  Expected values come from oracle.model's big integers
(pairs) and from the oracle's C msm_many over a small catalogue with net multiplicities as scalars (sums); the operands are those of
tests/point_sum_cases.py.  The host routines also run in a stand-alone program built with AddressSanitizer and UBSan.  No GPU needed."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cbind as C
from tests import point_mul_cases as PC
from tests import point_sum_cases as SC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD = -10          # ZKP_TB_BAD_STATEMENT
GROUP = 32           # (any value serves on the host: the ragged job's lengths are built around it)


@pytest.mark.parametrize("op", [SC.ADD, SC.SUB])
def test_pairs_equal_the_big_integer_model(op):
    a, b, valid = SC.pair_operands()
    want, want_st = SC.pair_expected(op)
    assert (want_st == ~valid).all() and (~valid).sum() >= 3 * len(SC.invalid_points())
    out, st = (T.point_add if op == SC.ADD else T.point_sub)(None, a, b, threads=5)
    assert (st == want_st).all()
    assert (out == want).all()
    assert not out[~valid].any()                                      # 32 zero bytes where an operand does not decode
    eng_out, eng_st = (T.point_add if op == SC.ADD else T.point_sub)(T.HostEngine(), a[:9], b[:9])
    assert (eng_out == want[:9]).all() and (eng_st == want_st[:9]).all()


def test_the_special_pairs():
    good = SC.valid_points()
    P = PC.enc_rows(list(good))
    Z = np.zeros_like(P)
    negP, st = T.point_neg(None, P)
    assert not st.any() and (negP == PC.enc_rows([SC.negated(p) for p in good])).all()
    for got in (T.point_add(None, P, negP), T.point_sub(None, P, P), T.point_add(None, Z, Z), T.point_sub(None, Z, Z)):
        assert not got[0].any() and not got[1].any()                  # P - P, 0 + 0: the identity, status 0
    for got in (T.point_add(None, P, Z), T.point_add(None, Z, P), T.point_sub(None, P, Z), T.point_neg(None, negP)):
        assert (got[0] == P).all() and not got[1].any()
    dbl, _ = T.point_add(None, P, P)
    two, _ = T.point_mul(None, PC.rows([2]), P)
    assert (dbl == two).all()
    neg_one, st = T.point_neg(None, P[3])                             # one row
    assert neg_one.shape == (1, 32) and (neg_one[0] == negP[3]).all()


@pytest.mark.parametrize("sa,sb", list(itertools.product((0, 1), repeat=2)))
@pytest.mark.parametrize("op", [SC.ADD, SC.SUB])
def test_strides_in_all_four_combinations(sa, sb, op):
    a, b, valid = SC.pair_operands()
    want, want_st = SC.pair_expected(op)
    n = len(a)
    a0, b0 = int(np.flatnonzero(valid)[7]), int(np.flatnonzero(valid)[11])     # the shared operands
    A = a if sa else a[a0:a0 + 1].copy()
    Bb = b if sb else b[b0:b0 + 1].copy()
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert T.lib().zkp_point_add_batch(None, n, T._p(A), sa, T._p(Bb), sb, op, 3, T._p(out), T._p(st)) == 0
    fa = a if sa else np.repeat(A, n, axis=0)
    fb = b if sb else np.repeat(Bb, n, axis=0)
    off = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    pts = np.ascontiguousarray(np.stack([fa, fb], axis=1).reshape(-1, 32))
    ref, ref_st = C.msm_many(off, SC.as_msm_job(off, None, np.tile([0, op], n)), np.arange(2 * n, dtype=np.uint32), pts, 0)
    assert (out == ref).all() and (st == ref_st).all()
    if sa and sb:
        assert (out == want).all() and (st == want_st).all()
    if sa != sb:                                                       # the Python wrapper derives the strides from the shapes
        got, gst = (T.point_add if op == SC.ADD else T.point_sub)(None, A if sa else A[0], Bb if sb else Bb[0])
        assert (got == out).all() and (gst == st).all()
    if not sb:                                                         # an invalid shared operand fails every output
        got, gst = T.point_add(None, a, PC.enc_rows(SC.invalid_points()[:1]))
        assert gst.all() and not got.any()


@pytest.mark.parametrize("op", [SC.ADD, SC.SUB])
def test_out_may_be_either_operand(op):
    a, b, _ = SC.pair_operands()
    want, want_st = SC.pair_expected(op)
    n = len(a)
    buf, st = a.copy(), np.zeros(n, np.uint8)
    assert T.lib().zkp_point_add_batch(None, n, T._p(buf), 1, T._p(b), 1, op, 4, T._p(buf), T._p(st)) == 0
    assert (buf == want).all() and (st == want_st).all()
    buf, st = b.copy(), np.zeros(n, np.uint8)
    assert T.lib().zkp_point_add_batch(None, n, T._p(a), 1, T._p(buf), 1, op, 4, T._p(buf), T._p(st)) == 0
    assert (buf == want).all() and (st == want_st).all()


def test_sums_on_a_ragged_job_equal_the_oracle():
    pts, bad = SC.catalogue()
    off, pidx, neg, flagged = SC.ragged_job(GROUP)
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    assert want_st.sum() == 1 and want_st[flagged] == 1 and not want[flagged].any()
    empty = np.diff(off.astype(np.int64)) == 0
    assert empty[[0, 1, -1]].all() and not want[empty].any() and not want_st[empty].any()
    for threads in (1, 3, 16):
        out, st = T.point_sum(None, off, pts, pidx, neg, threads=threads)
        assert (st == want_st).all() and (out == want).all(), threads
    # pidx == NULL: the same terms gathered
    out, st = T.point_sum(None, off, pts[pidx], None, neg, threads=3)
    assert (st == want_st).all() and (out == want).all()
    # neg == NULL: every term is added
    want_add, want_add_st = SC.segments_expected(off, pidx, None, pts)
    out, st = T.point_sum(None, off, pts, pidx, None, threads=2)
    assert (st == want_add_st).all() and (out == want_add).all() and (want_add != want).any()
    # the unit-scalar MSM callers built before gives the same bytes
    ref, ref_st = T.multiscalar_mul(None, off, SC.as_msm_job(off, pidx, neg), pidx, pts)
    assert (ref == want).all() and (ref_st == want_st).all()
    # a bad point that no term references flags nothing: the all-valid terms with the catalogue as it is
    keep = pidx != bad
    assert bad not in pidx[keep]
    o2 = np.array([0, int(keep.sum())], np.uint32)
    out, st = T.point_sum(None, o2, pts, pidx[keep], neg[keep])
    w2, w2_st = SC.segments_expected(o2, pidx[keep], neg[keep], pts)
    assert not st.any() and (out == w2).all() and not w2_st.any()


def test_thread_counts_give_the_same_bytes_on_segments_longer_than_the_split():
    pts, _ = SC.catalogue()
    lens = [3, 5000, 0, 70, 1, 900, 2]                                 # 5000 and 900 exceed a thread's share at 3 and 16 threads
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    _, pidx, neg = SC.single_segment(int(off[-1]), seed=4)
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    assert not want_st.any()
    for threads in (1, 3, 16):
        out, st = T.point_sum(None, off, pts, pidx, neg, threads=threads)
        assert (out == want).all() and not st.any(), threads
    # one segment that is the whole call, and the same with a point that does not decode in the last thread's piece
    o1, p1, n1 = SC.single_segment(4097, seed=6)
    want, _ = SC.segments_expected(o1, p1, n1, pts)
    for threads in (1, 3, 16):
        out, st = T.point_sum(None, o1, pts, p1, n1, threads=threads)
        assert (out == want).all() and not st.any(), threads
    p1[4090] = SC.catalogue()[1]
    for threads in (1, 16):
        out, st = T.point_sum(None, o1, pts, p1, n1, threads=threads)
        assert st[0] == 1 and not out.any(), threads
    # k copies of P against k P; P and -P alternating
    P = pts[2:3]
    k = 1000
    out, st = T.point_sum(None, np.array([0, k], np.uint32), P, np.zeros(k, np.uint32), None, threads=16)
    assert (out == T.point_mul(None, PC.rows([k]), P)[0]).all() and not st.any()
    out, st = T.point_sum(None, np.array([0, k], np.uint32), P, np.zeros(k, np.uint32), np.arange(k) % 2, threads=16)
    assert not out.any() and not st.any()


def test_no_ops_and_argument_errors_write_nothing():
    lib, p = T.lib(), T._p
    a, b, valid = SC.pair_operands()
    a, b = a[valid][:4].copy(), b[valid][:4].copy()
    out, st = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    # n = 0
    assert lib.zkp_point_add_batch(None, 0, None, 1, None, 1, SC.ADD, 0, None, None) == 0
    assert lib.zkp_point_sum_batch(None, 0, None, None, None, None, 0, 0, None, None) == 0
    got, gst = T.point_add(None, np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert got.shape == (0, 32) and gst.shape == (0,)
    got, gst = T.point_sum(None, np.zeros(4, np.uint32), np.zeros((0, 32), np.uint8))      # three empty sums, no points at all
    assert got.shape == (3, 32) and not got.any() and not gst.any()
    # NULL buffers, strides other than 0 / 1, an op other than the two, n > 2^31 - 1
    for args in ((None, 1, p(b), 1, SC.ADD, 0, p(out), p(st)), (p(a), 1, None, 1, SC.ADD, 0, p(out), p(st)),
                 (p(a), 1, p(b), 1, SC.ADD, 0, None, p(st)), (p(a), 1, p(b), 1, SC.ADD, 0, p(out), None),
                 (p(a), 2, p(b), 1, SC.ADD, 0, p(out), p(st)), (p(a), 1, p(b), 2, SC.SUB, 0, p(out), p(st)),
                 (p(a), 1, p(b), 1, 2, 0, p(out), p(st)), (p(a), 1, p(b), 1, -1, 0, p(out), p(st))):
        assert lib.zkp_point_add_batch(None, 4, *args) == T_BAD, args
    assert lib.zkp_point_add_batch(None, 2**31, p(a), 0, p(b), 0, SC.ADD, 0, p(out), p(st)) == T_BAD
    assert lib.zkp_point_add_batch(None, 0, None, 7, None, 1, SC.ADD, 0, None, None) == T_BAD      # (a bad stride is an error at any n)
    off, pidx, neg = np.arange(5, dtype=np.uint32), np.arange(4, dtype=np.uint32), np.zeros(4, np.uint8)
    sm = lambda *x: lib.zkp_point_sum_batch(None, *x)
    assert sm(4, p(off), p(pidx), p(neg), p(a), 4, 0, p(out), p(st)) == 0 and (out == a).all() and not st.any()     # (the good call)
    out[:] = 0
    assert sm(4, None, p(pidx), p(neg), p(a), 4, 0, p(out), p(st)) == T_BAD
    assert sm(4, p(off), p(pidx), p(neg), None, 4, 0, p(out), p(st)) == T_BAD
    assert sm(4, p(off), p(pidx), p(neg), p(a), 4, 0, None, p(st)) == T_BAD
    assert sm(4, p(off), p(pidx), p(neg), p(a), 4, 0, p(out), None) == T_BAD
    assert sm(4, p(off), p(pidx), p(neg), p(a), 3, 0, p(out), p(st)) == T_BAD                # index 3 out of range
    assert sm(4, p(off), None, p(neg), p(a), 3, 0, p(out), p(st)) == T_BAD                   # no pidx: n_points must equal T
    assert sm(4, p(off), None, p(neg), p(a), 5, 0, p(out), p(st)) == T_BAD
    assert sm(4, p(np.array([0, 2, 1, 3, 4], np.uint32)), p(pidx), p(neg), p(a), 4, 0, p(out), p(st)) == T_BAD     # decreasing
    assert sm(4, p(np.array([1, 1, 2, 3, 4], np.uint32)), p(pidx), p(neg), p(a), 4, 0, p(out), p(st)) == T_BAD     # off[0] != 0
    assert not out.any() and not st.any()
    with pytest.raises(ValueError):
        T.point_add(None, a, b[:3])
    with pytest.raises(ValueError):
        T.point_sum(None, off, a, pidx[:3])


def _example():
    spec = importlib.util.spec_from_file_location("elgamal_tally_batch", os.path.join(ROOT, "examples", "elgamal_tally_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_elgamal_tally_example_on_the_host_backend():
    n = 8
    votes = np.array([1, 0, 1, 1, 0, 0, 1, 0])
    r = _example().run(None, n, key=bytes(range(32)), votes=votes)
    assert r["accepted"] == n and r["rejected"] == n and r["decryption_verified"] and r["count"] == r["cast"] == 4
    # the sums against the oracle: S1 = (sum r_j) B through unit scalars, the result = 4 B
    off = np.array([0, n, 2 * n], np.uint32)
    want, st = C.msm_many(off, SC.as_msm_job(off, None, None), np.arange(2 * n, dtype=np.uint32), np.concatenate([r["C1"], r["C2"]]), 0)
    assert not st.any() and (want[0] == r["S1"][0]).all() and (want[1] == r["S2"][0]).all()
    four, _ = C.msm_many(np.array([0, 1], np.uint32), PC.rows([4]), np.zeros(1, np.uint32), PC.BASEPOINT_ROW, 0)
    assert (r["result"] == four).all()


def test_add_points_and_sum_points_under_sanitizers(tmp_path):
    """tests/host/point_sum_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: hostbk::add_points_n,
    sum_points_n, sum_points_partial and sum_points_finish on heap blocks of exactly the size a call may touch.  Exit 0, silent sanitizers,
    and every printed encoding equal to the oracle's."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "point_sum_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "point_sum_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    a, b, valid = SC.pair_operands()
    first = int(np.flatnonzero(valid)[5])                              # (row 0 supplies the shared operand: a valid point)
    pick = np.concatenate([[first], np.arange(0, 60), np.arange(len(a) - 25, len(a))])
    a, b = a[pick], b[pick]
    want_add, st_add = (x[pick] for x in SC.pair_expected(SC.ADD))
    want_sub, _ = (x[pick] for x in SC.pair_expected(SC.SUB))
    n = len(a)
    (tmp_path / "pairs.txt").write_text("".join(bytes(a[i]).hex() + " " + bytes(b[i]).hex() + "\n" for i in range(n)))
    pts, _ = SC.catalogue()
    off, pidx, neg, flagged = SC.ragged_job(8, cycles=2)
    (tmp_path / "sums.txt").write_text("%d %d %d\n%s\n%s\n%s\n%s\n" % (len(off) - 1, len(pidx), len(pts), " ".join(map(str, off)), " ".join(map(str, pidx)),
                                                                     " ".join(map(str, neg)), "\n".join(bytes(r).hex() for r in pts)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "pairs.txt"), str(tmp_path / "sums.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.split("\n")[:-1]
    pair_lines = [x.split()[1:] for x in lines if x.startswith("P ")]
    sum_lines = [x.split()[1:] for x in lines if x.startswith("S ")]
    assert len(pair_lines) == n and len(sum_lines) == len(off) - 1
    o2 = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    shared_pts = np.ascontiguousarray(np.stack([a, np.repeat(b[:1], n, axis=0)], axis=1).reshape(-1, 32))
    want_sh, st_sh = C.msm_many(o2, SC.as_msm_job(o2, None, np.tile([0, 1], n)), np.arange(2 * n, dtype=np.uint32), shared_pts, 0)
    for i, cols in enumerate(pair_lines):
        got = [bytes.fromhex(x) for x in cols[:4]]
        assert got == [bytes(want_add[i]), bytes(want_sub[i]), bytes(want_add[i]), bytes(want_sh[i])], i
        assert int(cols[4], 16) == int(st_add[i]) | (int(st_sh[i]) << 4), i
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    assert want_st[flagged] == 1
    for i, cols in enumerate(sum_lines):
        assert [bytes.fromhex(x) for x in cols[:3]] == [bytes(want[i])] * 3, i
        assert int(cols[3], 16) == int(want_st[i]), i

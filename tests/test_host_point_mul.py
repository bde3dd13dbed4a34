"""Batched Scalar * basepoint, Scalar * point and multiscalar products on the host backend (ctx == NULL): zkp_basepoint_mul_batch,
zkp_point_mul_batch and zkp_multiscalar_mul_batch run hostbk::mul_base_n / mul_points_n / msm_many -- the kernels' point formulas over the host
field -- on the host threads.  Expected values come from the oracle's C restatement (oracle.cbind.msm_many on the job off = arange(n + 1),
pidx = arange(n)), from oracle.model's big integers for a sample, and from RFC 9496 appendix A.1's sixteen multiples of the generator; the
operands are those of tests/point_mul_cases.py.  The host routines also run in a stand-alone program built with AddressSanitizer and UBSan.
No GPU needed."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests import point_mul_cases as PC
from tests.scalar_edge_cases import L
from tests.test_host_field import GENERATOR_MULTIPLES
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT, ZKP_VARTIME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD = -10          # ZKP_TB_BAD_STATEMENT


def test_rfc9496_generator_multiples_and_reduction_mod_l():
    want = PC.enc_rows([bytes.fromhex(h) for h in GENERATOR_MULTIPLES])
    for shift in (0, L, 15 * L):                                      # k, k + l and k + 15 l < 2^256 are the same multiple
        s = PC.rows([k + shift for k in range(16)])
        assert (T.basepoint_mul(None, s) == want).all(), shift
        for flags in (ZKP_CT, ZKP_VARTIME):
            out, st = T.point_mul(None, s, PC.BASEPOINT_ROW, flags)
            assert (out == want).all() and not st.any(), (shift, flags)
    assert not T.basepoint_mul(None, PC.rows([0, L, 2 * L])).any()     # the zero scalar: 32 zero bytes


def test_basepoint_mul_over_the_scalar_operands_equals_the_oracle():
    s = PC.base_operands()
    assert len(s) >= 148 + 7 + 10
    assert (T.basepoint_mul(None, s, threads=4) == PC.base_expected()).all()
    assert (T.basepoint_mul(T.HostEngine(), s[:3]) == PC.base_expected()[:3]).all()


@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
def test_point_mul_over_the_pair_operands_equals_the_oracle(flags):
    s, p, valid = PC.pair_operands()
    want, want_st = PC.pair_expected()
    assert (want_st == ~valid).all() and (~valid).sum() >= 2 * len(PC.invalid_points())
    out, st = T.point_mul(None, s, p, flags, threads=5)
    assert (st == want_st).all()
    assert (out == want).all()
    assert not out[~valid].any()                                      # 32 zero bytes where the point does not decode
    ident = (p == 0).all(axis=1)
    assert ident.any() and not out[ident].any() and not st[ident].any()   # the identity point: zero bytes, status 0


def test_a_sample_equals_the_big_integer_model():
    s, p, valid = PC.pair_operands()
    pick = [i for i in range(0, len(s), 37) if valid[i]][:12]
    out, _ = T.point_mul(None, s[pick], p[pick])
    base = T.basepoint_mul(None, s[pick])
    for k, i in enumerate(pick):
        v = int.from_bytes(bytes(s[i]), "little")
        assert bytes(out[k]) == M.ristretto_encode(M.pt_mul(v % L, M.ristretto_decode(bytes(p[i])))), i
        assert bytes(base[k]) == M.ristretto_encode(M.pt_mul(v % L, M.BASEPOINT)), i


@pytest.mark.parametrize("ss,ps", list(itertools.product((0, 1), repeat=2)))
@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
def test_strides_in_all_four_combinations(ss, ps, flags):
    s, p, valid = PC.pair_operands()
    n = len(s)
    s0, p0 = 5, int(np.flatnonzero(valid)[3])                          # the shared operands
    S = s if ss else s[s0:s0 + 1].copy()
    P = p if ps else p[p0:p0 + 1].copy()
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    rc = T.lib().zkp_point_mul_batch(None, n, T._p(S), ss, T._p(P), ps, flags, 3, T._p(out), T._p(st))
    assert rc == 0
    want, want_st = C.msm_many(np.arange(n + 1, dtype=np.uint32), s if ss else np.repeat(S, n, axis=0), np.arange(n, dtype=np.uint32),
                               p if ps else np.repeat(P, n, axis=0), 1)
    assert (out == want).all() and (st == want_st).all()
    # the Python wrapper derives the strides from the shapes
    if ss or ps:
        got, gst = T.point_mul(None, S if ss else S[0], P if ps else P, flags)
        assert (got == out).all() and (gst == st).all()
    else:
        got, gst = T.point_mul(None, S[0], P[0], flags)
        assert got.shape == (1, 32) and (got[0] == want[0]).all()
    # an invalid shared point fails every output
    if not ps:
        bad = PC.enc_rows(PC.invalid_points()[:1])
        got, gst = T.point_mul(None, S, bad, flags)
        assert gst.all() and not got.any()


def test_out_may_be_points():
    s, p, _ = PC.pair_operands()
    want, want_st = PC.pair_expected()
    for flags in (ZKP_CT, ZKP_VARTIME):
        buf, st = p.copy(), np.zeros(len(p), np.uint8)
        assert T.lib().zkp_point_mul_batch(None, len(s), T._p(s), 1, T._p(buf), 1, flags, 4, T._p(buf), T._p(st)) == 0
        assert (buf == want).all() and (st == want_st).all()


def test_identities_with_the_basepoint_and_the_inverse():
    s = PC.base_operands()
    out, st = T.point_mul(None, s, PC.BASEPOINT_ROW)
    assert (out == T.basepoint_mul(None, s)).all() and not st.any()
    # s^-1 (s P) = P for s != 0 mod l
    sc, p, valid = PC.pair_operands()
    keep = valid & np.array([int.from_bytes(bytes(r), "little") % L != 0 for r in sc])
    sc, p = sc[keep], p[keep]
    sp, _ = T.point_mul(None, sc, p)
    back, st = T.point_mul(None, T.scalar_invert(None, sc), sp)
    assert (back == p).all() and not st.any()


def ragged_job(seed=3, n_msm=41, n_points=23):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, size=n_msm)
    lens[[0, 7, n_msm - 1]] = 0                                        # empty ranges: first, inside, last
    lens[11] = 17
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    t = int(off[-1])
    vals = PC.scalar_values()
    sc = PC.rows([vals[int(i)] for i in rng.integers(0, len(vals), size=t)])
    good = PC.valid_points()
    pts = [good[i % len(good)] for i in range(n_points - 1)] + [PC.invalid_points()[2]]
    pidx = rng.integers(0, n_points - 1, size=t).astype(np.uint32)
    pidx[int(off[20])] = n_points - 1                                  # one MSM names the point that does not decode
    return off, sc, pidx, PC.enc_rows(pts)


@pytest.mark.parametrize("flags", [ZKP_CT, ZKP_VARTIME])
def test_multiscalar_mul_on_a_ragged_job_with_empty_ranges_equals_the_oracle(flags):
    off, sc, pidx, pts = ragged_job()
    want, want_st = C.msm_many(off, sc, pidx, pts, flags)
    assert want_st.sum() == 1 and not want[0].any()
    for threads in (1, 4):
        out, st = T.multiscalar_mul(None, off, sc, pidx, pts, flags, threads=threads)
        assert (out == want).all() and (st == want_st).all()
    # more MSMs than a thread's share: the per-thread ranges rebase their offsets
    big_off = np.arange(0, 2 * 250 + 1, 2, dtype=np.uint32)
    s, p, _ = PC.pair_operands()
    out, st = T.multiscalar_mul(None, big_off, s[:500], np.arange(500, dtype=np.uint32) % 7, p[:7], flags, threads=8)
    want, want_st = C.msm_many(big_off, s[:500], np.arange(500, dtype=np.uint32) % 7, p[:7], flags)
    assert (out == want).all() and (st == want_st).all()


def test_no_ops_and_argument_errors_write_nothing():
    lib, p = T.lib(), T._p
    s, pts, _ = PC.pair_operands()
    s, pts = s[:4].copy(), pts[:4].copy()
    out, st = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    off, pidx = np.arange(5, dtype=np.uint32), np.arange(4, dtype=np.uint32)
    # n = 0
    assert lib.zkp_basepoint_mul_batch(None, 0, None, 0, None) == 0
    assert lib.zkp_point_mul_batch(None, 0, None, 1, None, 1, ZKP_CT, 0, None, None) == 0
    assert lib.zkp_multiscalar_mul_batch(None, 0, None, None, None, None, 0, ZKP_CT, 0, None, None) == 0
    assert T.basepoint_mul(None, np.zeros((0, 32), np.uint8)).shape == (0, 32)
    # NULL buffers
    assert lib.zkp_basepoint_mul_batch(None, 4, None, 0, p(out)) == T_BAD and lib.zkp_basepoint_mul_batch(None, 4, p(s), 0, None) == T_BAD
    for args in ((None, 1, p(pts), 1, ZKP_CT, 0, p(out), p(st)), (p(s), 1, None, 1, ZKP_CT, 0, p(out), p(st)),
                 (p(s), 1, p(pts), 1, ZKP_CT, 0, None, p(st)), (p(s), 1, p(pts), 1, ZKP_CT, 0, p(out), None),
                 # strides other than 0 / 1, flags other than ZKP_CT / ZKP_VARTIME, n > 2^31 - 1
                 (p(s), 2, p(pts), 1, ZKP_CT, 0, p(out), p(st)), (p(s), 1, p(pts), 2, ZKP_CT, 0, p(out), p(st)),
                 (p(s), 1, p(pts), 1, 2, 0, p(out), p(st)), (p(s), 1, p(pts), 1, -1, 0, p(out), p(st))):
        assert lib.zkp_point_mul_batch(None, 4, *args) == T_BAD, args
    assert lib.zkp_point_mul_batch(None, 2**31, p(s), 0, p(pts), 0, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert lib.zkp_basepoint_mul_batch(None, 2**31, p(s), 0, p(out)) == T_BAD
    assert lib.zkp_point_mul_batch(None, 0, None, 7, None, 1, ZKP_CT, 0, None, None) == T_BAD      # (a bad stride is an error at any n)
    ms = lambda *a: lib.zkp_multiscalar_mul_batch(None, *a)
    assert ms(4, None, p(s), p(pidx), p(pts), 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(off), None, p(pidx), p(pts), 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(off), p(s), None, p(pts), 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(off), p(s), p(pidx), None, 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(off), p(s), p(pidx), p(pts), 4, ZKP_CT, 0, None, p(st)) == T_BAD
    assert ms(4, p(off), p(s), p(pidx), p(pts), 4, ZKP_CT, 0, p(out), None) == T_BAD
    assert ms(4, p(off), p(s), p(pidx), p(pts), 4, 5, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(off), p(s), p(pidx), p(pts), 3, ZKP_CT, 0, p(out), p(st)) == T_BAD              # pidx 3 out of range
    assert ms(4, p(np.array([0, 2, 1, 3, 4], np.uint32)), p(s), p(pidx), p(pts), 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert ms(4, p(np.array([1, 1, 2, 3, 4], np.uint32)), p(s), p(pidx), p(pts), 4, ZKP_CT, 0, p(out), p(st)) == T_BAD
    assert not out.any() and not st.any()
    with pytest.raises(ValueError):
        T.point_mul(None, s, pts[:3])


def test_one_and_sixteen_threads_give_the_same_bytes():
    s, p, _ = PC.pair_operands()
    a, sa = T.point_mul(None, s, p, threads=1)
    b, sb = T.point_mul(None, s, p, threads=16)
    assert (a == b).all() and (sa == sb).all()
    assert (T.basepoint_mul(None, s, threads=1) == T.basepoint_mul(None, s, threads=16)).all()


def _example():
    spec = importlib.util.spec_from_file_location("keygen_vrf_batch", os.path.join(ROOT, "examples", "keygen_vrf_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_keygen_vrf_example_on_the_host_backend():
    n = 24
    r = _example().run(None, n, key=bytes(range(32)))
    assert r["accepted"] == n and all(v == n for v in r["rejected"].values()) and len(r["rejected"]) == 4
    iota = np.arange(n + 1, dtype=np.uint32)
    want_pk, _ = C.msm_many(iota, r["sk"], np.zeros(n, np.uint32), PC.BASEPOINT_ROW, 1)
    want_g, _ = C.msm_many(iota, r["sk"], np.arange(n, dtype=np.uint32), r["H"], 1)
    assert (r["pk"] == want_pk).all() and (r["G"] == want_g).all()
    assert len({bytes(k) for k in r["pk"]}) == n                        # distinct keys


def test_mul_base_and_mul_points_under_sanitizers(tmp_path):
    """tests/host/point_mul_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: the edge operands
    through hostbk::mul_base_n / mul_points_n on heap blocks of exactly the size a call may touch.  Exit 0, silent sanitizers, and every
    printed encoding equal to the oracle's."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "point_mul_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "point_mul_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    s, p, valid = PC.pair_operands()
    want, want_st = PC.pair_expected()
    pick = np.concatenate([np.arange(0, 40), np.flatnonzero(~valid)[:12], np.flatnonzero(~valid)[:12] + 1, np.arange(len(s) - 6, len(s))])
    pick = np.unique(pick)
    pick = np.concatenate([[int(np.flatnonzero(valid)[2])], pick])     # (row 0 supplies the shared operands: a valid point)
    s, p, want, want_st = s[pick], p[pick], want[pick], want_st[pick]
    n = len(s)
    (tmp_path / "pairs.txt").write_text("".join(bytes(s[i]).hex() + " " + bytes(p[i]).hex() + "\n" for i in range(n)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "pairs.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == n
    iota = np.arange(n + 1, dtype=np.uint32)
    want_base, _ = C.msm_many(iota, s, np.zeros(n, np.uint32), PC.BASEPOINT_ROW, 1)
    want_sp, _ = C.msm_many(iota, s, np.zeros(n, np.uint32), p[:1], 1)
    want_ss, st_ss = C.msm_many(iota, np.repeat(s[:1], n, axis=0), np.arange(n, dtype=np.uint32), p, 1)
    for i, line in enumerate(lines):
        cols = line.split()
        got = [bytes.fromhex(x) for x in cols[:6]]
        assert got == [bytes(want_base[i]), bytes(want[i]), bytes(want[i]), bytes(want[i]), bytes(want_sp[i]), bytes(want_ss[i])], i
        assert int(cols[6], 16) == int(want_st[i]) | (int(st_ss[i]) << 4), i

"""Bounded discrete logarithms to the basepoint on the host backend (ctx == NULL): zkp_basepoint_dlog_batch runs hostbk::dlog_base_range -- the
baby-step / giant-step of dlog.h over the kernels' point formulas and the host field -- on the host threads.  The operands are those of
tests/dlog_cases.py: encode(k B) from the oracle for integers the test chose, and the expected output is k.  The host routines also run in a
stand-alone program built with AddressSanitizer and UBSan.  No GPU needed."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dlog_cases as DC
from tests import point_mul_cases as PC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD = -10          # ZKP_TB_BAD_STATEMENT
HOST_SHAPES = [(4, 1), (4, 3), (4, 4), (4, 5), (4, 12), (4, 20), (8, 1), (8, 7), (8, 8), (8, 9), (8, 16), (8, 20)]


@pytest.fixture
def baby_bits():
    before = T.get_dlog_baby_bits()

    def use(bb):
        T.set_dlog_baby_bits(bb)
        return bb
    yield use
    T.set_dlog_baby_bits(before)


def plan():
    lib = T.lib()
    return int(lib.zkp_dlog_group()), int(lib.zkp_dlog_chunk())


def test_the_plan_is_what_the_cases_are_built_around():
    group, chunk = plan()
    assert group >= 2 and chunk >= 2
    assert T.lib().zkp_dlog_slice_chunks(1) >= 1 and T.lib().zkp_dlog_slice_chunks(2**31 - 1) == 1
    assert 4 <= T.get_dlog_baby_bits() <= 22


@pytest.mark.parametrize("bb,bits", HOST_SHAPES)
def test_the_cases_on_the_host_backend(baby_bits, bb, bits):
    baby_bits(bb)
    group, chunk = plan()
    pts, want_k, want_st = DC.operands(bb, bits, chunk)
    assert (want_st == DC.FOUND).sum() >= 2 and (want_st == DC.INVALID).sum() >= 3 and (want_st == DC.NOT_FOUND).sum() >= 4
    for threads in (1, 5):
        k, st = T.basepoint_dlog(None, pts, bits, threads=threads)
        assert (st == want_st).all(), (threads, np.flatnonzero(st != want_st))
        assert (k == want_k).all(), (threads, np.flatnonzero(k != want_k))
    assert not k[want_st != DC.FOUND].any()
    # what the call found is what the oracle encodes
    assert (DC.encode_multiples(k[st == DC.FOUND]) == pts[st == DC.FOUND]).all()


def test_one_point_is_spread_over_the_threads_by_giant_step_ranges(baby_bits):
    baby_bits(4)
    bits = 18                                                          # 2^14 giant steps: 64 groups of 256, split over up to 16 threads
    ks = [0, 1, 15, 16, (1 << 18) - 1, (1 << 17) + 16 * 256 * 3, 16 * 256 * 4 - 1, 16 * 256 * 4]
    for threads in (1, 3, 16):
        for k in ks:
            got, st = T.basepoint_dlog(None, DC.encode_multiples([k]), bits, threads=threads)
            assert st[0] == DC.FOUND and int(got[0]) == k, (threads, k)
        got, st = T.basepoint_dlog(None, DC.encode_multiples([1 << 18]), bits, threads=threads)
        assert st[0] == DC.NOT_FOUND and got[0] == 0
        got, st = T.basepoint_dlog(None, PC.enc_rows(PC.invalid_points()[:1]), bits, threads=threads)
        assert st[0] == DC.INVALID and got[0] == 0


def test_tables_of_two_sizes_give_the_same_answers(baby_bits):
    _, chunk = plan()
    pts, want_k, want_st = DC.operands(8, 16, chunk)
    for bb in (4, 8, 11, 4):                                          # (4 again: the table kept from the first round)
        baby_bits(bb)
        k, st = T.basepoint_dlog(None, pts, 16, threads=4)
        assert (k == want_k).all() and (st == want_st).all(), bb


def test_the_identity_and_the_ends_of_every_range(baby_bits):
    baby_bits(4)
    zero = np.zeros((1, 32), np.uint8)
    for bits in (1, 2, 4, 5, 9, 20):
        k, st = T.basepoint_dlog(None, zero, bits)
        assert st[0] == DC.FOUND and k[0] == 0
        top = (1 << bits) - 1
        k, st = T.basepoint_dlog(None, DC.encode_multiples([top, top + 1, 1]), bits)
        assert st.tolist() == [DC.FOUND, DC.NOT_FOUND, DC.FOUND] and k.tolist() == [top, 0, 1], bits


def test_no_ops_and_argument_errors_write_nothing(baby_bits):
    lib, p = T.lib(), T._p
    pts = DC.encode_multiples([3, 4])
    out, st = np.full(2, 77, np.uint64), np.full(2, 9, np.uint8)
    assert lib.zkp_basepoint_dlog_batch(None, 0, None, 8, None, None, 0) == 0
    k, s = T.basepoint_dlog(None, np.zeros((0, 32), np.uint8), 8)
    assert k.shape == (0,) and s.shape == (0,)
    for args in ((None, 8, p(out), p(st)), (p(pts), 8, None, p(st)), (p(pts), 8, p(out), None), (p(pts), 0, p(out), p(st)),
                 (p(pts), 49, p(out), p(st)), (p(pts), 2**32 - 1, p(out), p(st))):
        assert lib.zkp_basepoint_dlog_batch(None, 2, *args, 0) == T_BAD, args
    assert lib.zkp_basepoint_dlog_batch(None, 2**31, p(pts), 8, p(out), p(st), 0) == T_BAD
    assert lib.zkp_basepoint_dlog_batch(None, 0, None, 0, None, None, 0) == T_BAD                  # (bits out of range is an error at any n)
    assert (out == 77).all() and (st == 9).all()
    before = T.get_dlog_baby_bits()
    for bad in (0, 3, 23, 64):
        assert lib.zkp_toolbox_set_dlog_baby_bits(bad) == T_BAD
    assert T.get_dlog_baby_bits() == before
    with pytest.raises(ValueError):
        T.basepoint_dlog(None, np.zeros((2, 31), np.uint8), 8)


def _example():
    spec = importlib.util.spec_from_file_location("elgamal_amounts_batch", os.path.join(ROOT, "examples", "elgamal_amounts_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_elgamal_amounts_example_on_the_host_backend():
    n, bits = 8, 10
    amounts = [0, 1, 1023, 1024, 512, 33, 7, 2000]                     # 1024 and 2000 are not below 2^10
    r = _example().run(None, n, bits, key=bytes(range(32)), amounts=amounts)
    assert r["accepted"] == n and r["rejected"] == n and r["match"]
    assert r["status"].tolist() == [0, 0, 0, 2, 0, 0, 0, 2]
    assert r["recovered"].tolist() == [0, 1, 1023, 0, 512, 33, 7, 0]
    assert (r["aB"] == DC.encode_multiples(amounts)).all()             # C2 - Z is a B: the oracle's encoding


def test_dlog_under_sanitizers(tmp_path):
    """tests/host/dlog_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: hostbk::dlog_base_n at two
    table sizes and dlog_base_range over three ranges per point, on heap blocks of exactly the size a call may touch.  Exit 0, silent
    sanitizers, and every printed logarithm the integer the test chose."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "dlog_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "dlog_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                    "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    _, chunk = plan()
    bits, bb, bb2 = 11, 4, 6
    pts, want_k, want_st = DC.operands(bb, bits, chunk)
    (tmp_path / "points.txt").write_text("".join(bytes(r).hex() + "\n" for r in pts))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "points.txt"), str(bits), str(bb), str(bb2)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = [[int(x) for x in ln.split()] for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == len(pts)
    for i, cols in enumerate(lines):
        assert cols == [int(want_k[i]), int(want_st[i])] * 3, i

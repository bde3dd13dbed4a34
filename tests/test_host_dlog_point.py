"""Bounded discrete logarithms to a base of the caller's, unsigned and signed, on the host backend (ctx == NULL): zkp_point_dlog_batch runs
hostbk::dlog_point_range -- the baby-step / giant-step of dlog.h with a table per (base, size), the signed walk outward from k = 0 -- on the host
threads.  The operands are those of tests/dlog_point_cases.py: encode(k G) from the oracle for integers the test chose, and the expected output
is k.  The launch order zkp_dlog_slice_order is checked as arithmetic, and the host routines also run in a stand-alone program built with
AddressSanitizer and UBSan.  No GPU needed."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dlog_cases as DC
from tests import dlog_point_cases as PD
from tests import point_mul_cases as PC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD, T_INVALID = -10, -11          # ZKP_TB_BAD_STATEMENT, ZKP_TB_INVALID_POINT
SIGNED = 1


@pytest.fixture
def baby_bits():
    before = T.get_dlog_baby_bits()

    def use(bb):
        T.set_dlog_baby_bits(bb)
        return bb
    yield use
    T.set_dlog_baby_bits(before)


def chunk():
    return int(T.lib().zkp_dlog_chunk())


def check(name, pts, bits, signed, want_k, want_st, threads):
    k, st = T.point_dlog(None, PD.base(name), pts, bits, signed=signed, threads=threads)
    assert k.dtype == (np.int64 if signed else np.uint64)
    assert (st == want_st).all(), (name, bits, signed, threads, np.flatnonzero(st != want_st))
    assert (k == want_k).all(), (name, bits, signed, threads, np.flatnonzero(k != want_k))
    return k, st


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("bb", [4, 8])
@pytest.mark.parametrize("name", PD.BASES)
def test_the_cases_on_the_host_backend(baby_bits, name, bb, signed):
    baby_bits(bb)
    for bits in sorted({1, 2, bb - 1, bb, bb + 1, bb + 6, bb + 11}):
        pts, want_k, want_st = PD.operands(name, bb, bits, chunk(), None, signed)
        assert (want_st == PD.FOUND).sum() >= 2 and (want_st == PD.INVALID).sum() >= 3 and (want_st == PD.NOT_FOUND).sum() >= 4
        for threads in (1, 4):
            k, st = check(name, pts, bits, signed, want_k, want_st, threads)
        assert not k[want_st != PD.FOUND].any()
        assert (PD.encode_multiples(name, k[st == PD.FOUND]) == pts[st == PD.FOUND]).all()       # what was found is what the oracle encodes


@pytest.mark.parametrize("bb,bits", [(4, 1), (4, 5), (4, 12), (8, 8), (8, 16)])
def test_base_b_gives_the_bytes_of_basepoint_dlog(baby_bits, bb, bits):
    baby_bits(bb)
    pts, want_k, want_st = DC.operands(bb, bits, chunk())
    for threads in (1, 4):
        k0, st0 = T.basepoint_dlog(None, pts, bits, threads=threads)
        k, st = T.point_dlog(None, PC.BASEPOINT, pts, bits, threads=threads)
        assert k.tobytes() == k0.tobytes() and st.tobytes() == st0.tobytes()
        assert (k == want_k).all() and (st == want_st).all()


def test_signed_bits_1_is_minus_one_and_zero(baby_bits):
    baby_bits(4)
    for name in PD.BASES:
        k, st = T.point_dlog(None, PD.base(name), PD.encode_multiples(name, [-1, 0, 1, -2]), 1, signed=True)
        assert st.tolist() == [PD.FOUND, PD.FOUND, PD.NOT_FOUND, PD.NOT_FOUND] and k.tolist() == [-1, 0, 0, 0], name


def test_one_point_is_spread_over_the_threads_in_signed_mode(baby_bits):
    baby_bits(4)
    bits = 18                                                          # 2^14 giant steps: 64 groups of 256, split over up to 16 threads
    half = 1 << 17
    seg = 16 * 256 * 4                                                 # the k covered by one of 16 threads' segments
    ks = [0, 1, -1, 15, -16, half - 1, -half, seg - 1 - half, seg - half, -seg, seg, 16 * 256 * 3 + 5, -(16 * 256 * 3) - 5]
    for threads in (1, 3, 16):
        for k0 in ks:
            got, st = T.point_dlog(None, PD.base("H"), PD.encode_multiples("H", [k0]), bits, signed=True, threads=threads)
            assert st[0] == PD.FOUND and int(got[0]) == k0, (threads, k0)
        for k0 in (half, -half - 1):
            got, st = T.point_dlog(None, PD.base("H"), PD.encode_multiples("H", [k0]), bits, signed=True, threads=threads)
            assert st[0] == PD.NOT_FOUND and got[0] == 0, (threads, k0)
        got, st = T.point_dlog(None, PD.base("H"), PC.enc_rows(PC.invalid_points()[:1]), bits, signed=True, threads=threads)
        assert st[0] == PD.INVALID and got[0] == 0


def test_a_ninth_base_evicts_the_least_recently_used_table_and_answers_stay_right(baby_bits):
    baby_bits(4)
    bits = 9
    ks = [0, 1, -1, 17, -200, 255, -256]
    bases = [PD.base(n) for n in PD.BASES] + PD.other_bases(7)        # ten distinct bases over a cache of eight tables
    mult = {i: (1, 7, None)[i] if i < 3 else 100 + i - 3 for i in range(len(bases))}
    for rnd in range(2):                                               # the second round meets every table evicted and rebuilt
        for i, b in enumerate(bases):
            if mult[i] is None:
                pts = PD.encode_multiples("H", ks)
            else:
                pts = DC.encode_multiples([(k * mult[i]) % PD.L for k in ks])
            k, st = T.point_dlog(None, b, pts, bits, signed=True, threads=2)
            assert not st.any() and k.tolist() == ks, (rnd, i)


@pytest.mark.parametrize("n_slices", [1, 2, 3, 4, 7, 64])
def test_the_slice_order_is_a_permutation_outward_from_the_zero_slice(n_slices):
    lib = T.lib()
    unsigned = [int(lib.zkp_dlog_slice_order(n_slices, 0, i)) for i in range(n_slices)]
    assert unsigned == list(range(n_slices))
    signed = [int(lib.zkp_dlog_slice_order(n_slices, SIGNED, i)) for i in range(n_slices)]
    assert sorted(signed) == list(range(n_slices))
    z = n_slices // 2
    assert signed[0] == z                                              # the slice that holds k' = 2^(bits - 1), i.e. k = 0
    assert signed == PD.slice_order(n_slices, True)
    dist = [abs(s - z) for s in signed]
    assert dist == sorted(dist)                                        # ascending distance from it
    both = min(z, n_slices - 1 - z)
    for i in range(1, 2 * both, 2):                                    # alternately below and above while both sides last
        assert signed[i] == z - (i + 1) // 2 and signed[i + 1] == z + (i + 1) // 2


def test_a_signed_slice_is_a_power_of_two_so_that_the_zero_slice_starts_at_zero():
    lib = T.lib()
    for n in (1, 2, 3, 60, 300, 4096, 5000, 2**20, 2**20 + 1, 2**31 - 1):
        per, sper = int(lib.zkp_dlog_slice_chunks(n)), int(lib.zkp_dlog_slice_chunks_signed(n))
        assert sper & (sper - 1) == 0 and sper <= per < 2 * sper
        for chunks in (1, 2, 64, 2**20, 2**39):                        # the chunks of a point are a power of two
            n_slices = (chunks + sper - 1) // sper
            if n_slices > 1:
                assert (n_slices // 2) * sper == chunks // 2           # k' = 2^(bits - 1) is the first step of slice n_slices / 2


def test_no_ops_and_argument_errors_write_nothing(baby_bits):
    baby_bits(4)
    lib, p = T.lib(), T._p
    H = PC.enc_rows([PD.base("H")])
    pts = PD.encode_multiples("H", [3, 4])
    out, st = np.full(2, 77, np.uint64), np.full(2, 9, np.uint8)
    assert lib.zkp_point_dlog_batch(None, p(H), 0, None, 8, 0, None, None, 0) == 0
    k, s = T.point_dlog(None, PD.base("H"), np.zeros((0, 32), np.uint8), 8, signed=True)
    assert k.shape == (0,) and s.shape == (0,) and k.dtype == np.int64
    bad_base = PC.enc_rows(PC.invalid_points()[:1])
    identity = np.zeros((1, 32), np.uint8)
    assert lib.zkp_point_dlog_batch(None, p(bad_base), 2, p(pts), 8, 0, p(out), p(st), 0) == T_INVALID
    assert lib.zkp_point_dlog_batch(None, p(identity), 2, p(pts), 8, 0, p(out), p(st), 0) == T_BAD
    assert lib.zkp_point_dlog_batch(None, None, 2, p(pts), 8, 0, p(out), p(st), 0) == T_BAD
    for args in ((None, 8, 0, p(out), p(st)), (p(pts), 8, 0, None, p(st)), (p(pts), 8, 0, p(out), None), (p(pts), 0, 0, p(out), p(st)),
                 (p(pts), 49, SIGNED, p(out), p(st)), (p(pts), 8, 2, p(out), p(st)), (p(pts), 8, 3, p(out), p(st)), (p(pts), 8, -1, p(out), p(st))):
        assert lib.zkp_point_dlog_batch(None, p(H), 2, *args, 0) == T_BAD, args
    assert lib.zkp_point_dlog_batch(None, p(H), 2**31, p(pts), 8, 0, p(out), p(st), 0) == T_BAD
    assert lib.zkp_point_dlog_batch(None, p(H), 0, None, 0, 0, None, None, 0) == T_BAD           # (bits out of range is an error at any n)
    assert lib.zkp_point_dlog_batch(None, p(H), 0, None, 8, 2, None, None, 0) == T_BAD           # (and so is an unknown flag)
    assert (out == 77).all() and (st == 9).all()
    with pytest.raises(ValueError):
        T.point_dlog(None, b"short", pts, 8)


def _example():
    spec = importlib.util.spec_from_file_location("net_balances_batch", os.path.join(ROOT, "examples", "net_balances_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_net_balances_example_on_the_host_backend():
    n, bits = 6, 10
    transfers = [[5, -5, 0], [100, -300, 1], [511, 0, 0], [256, 256, 0], [-512, 0, 0], [-500, -13, 0]]       # 512 and -513 are outside [-512, 512)
    r = _example().run(None, n, bits, key=bytes(range(32)), transfers=transfers)
    assert r["accepted"] == n and r["rejected"] == n and r["match"]
    assert r["status"].tolist() == [0, 0, 0, 2, 0, 2]
    assert r["recovered"].tolist() == [0, -199, 511, 0, -512, 0]
    assert bytes(r["H"][0]) == bytes(T.hash_from_bytes_sha512(None, [_example().H_LABEL])[0])
    d = _example().run(None, 4, 12, key=bytes(range(32)))              # the default ledger: the last account is out of range
    assert d["match"] and d["status"].tolist()[-1] == 2 and not d["status"][:-1].any()


def test_dlog_point_under_sanitizers(tmp_path):
    """tests/host/dlog_point_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: hostbk::dlog_point_n for
    two bases in both modes and dlog_point_range over three ranges per point, on heap blocks of exactly the size a call may touch.  Exit 0,
    silent sanitizers, and every printed logarithm the integer the test chose."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "dlog_point_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "dlog_point_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                    "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    bits, bb = 14, 4                                                   # 2^10 giant steps: four groups, so the signed order is not the plain one
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in ("G7", "H"):
        want = {}
        lines = [PD.base(name).hex() + "\n"]
        for signed in (False, True):
            pts, want_k, want_st = PD.operands(name, bb, bits, chunk(), None, signed)
            want[signed] = (want_k, want_st)
            lines.append("%d %d\n" % (int(signed), len(pts)))
            lines += [bytes(r).hex() + "\n" for r in pts]
        (tmp_path / "points.txt").write_text("".join(lines))
        r = subprocess.run([str(exe), str(tmp_path / "points.txt"), str(bits), str(bb)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows = [[int(x) for x in ln.split()] for ln in r.stdout.split("\n")[:-1]]
        assert len(rows) == len(want[False][0]) + len(want[True][0])
        i = 0
        for signed in (False, True):
            for wk, ws in zip(*want[signed]):
                assert rows[i] == [int(signed)] + [int(wk), int(ws)] * 2, (name, signed, i)
                i += 1

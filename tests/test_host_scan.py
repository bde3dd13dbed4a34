"""Segmented prefix sums and products of scalars and running sums of points on the host backend (no GPU): toolbox.scalar_cumsum / scalar_cumprod /
scalar_powers / point_cumsum with eng = None are hostbk::sc_scan_n and hostbk::point_scan_n, which cut the TERM axis over their threads: a stretch
is scanned from the identity, the stretch totals serially, and every thread fixes up its first run.  Every row is compared with Python integers
mod l, and every point row with (the sum of the known logarithms) B and with the existing host point_sum over the prefix segments
(tests/scan_cases.py), for 1, 5 and 40 threads, both ops and both modes; then the same code runs in a stand-alone program under AddressSanitizer
and UBSan."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import scan_cases as SC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (1, 5, 40)
BAD_STATEMENT = -10


@pytest.fixture(scope="module")
def G():
    from zkp_amd.engine import load_library
    g = int(load_library().zkp_sc_scan_group())             # pure arithmetic: no context, no GPU
    assert g >= 8
    return g


@pytest.fixture(scope="module")
def GP():
    from zkp_amd.engine import load_library
    g = int(load_library().zkp_scan_points_group())
    assert g >= 8
    return g


def sc_run(jb, exclusive, threads):
    op, off, a, aidx = jb
    return T.scalar_scan(None, op, off, SC.rows(a), aidx, exclusive, threads)


def sc_check(jb, threads=THREADS):
    for exclusive in SC.MODES:
        want = SC.sc_expected(*jb, exclusive=exclusive)
        for t in threads:
            assert SC.ints(sc_run(jb, exclusive, t)) == want, (jb[0], exclusive, t)


def pt_check(jb, threads=THREADS):
    off, pidx, neg = jb
    for exclusive in SC.MODES:
        want, wst = SC.pt_expected(off, pidx, neg, exclusive)
        for t in threads:
            out, st = T.point_cumsum(None, off, SC.catalogue(), pidx, neg, exclusive, t)
            assert (st == wst).all() and (out == want).all(), (exclusive, t)


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_single_segments_around_the_unit_edges(G, op):
    for n in SC.single_lengths(G):
        sc_check(SC.sc_job(op, [n], seed=n))


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_shapes(G, op):
    for k, (name, lens) in enumerate(SC.shapes(G).items()):
        sc_check(SC.sc_job(op, lens, seed=10 + k))


def test_scalar_long_segment_that_many_threads_cut(G):
    for op in SC.OPS:
        sc_check(SC.sc_job(op, [3, 40 * 64 + 11, 0, 70, 1], seed=3), threads=(1, 7, 40))


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_edge_values_as_operands(G, op):
    for shift in range(0, len(SC.EDGES), 7):
        sc_check(SC.sc_edge_rotation(op, G, shift), threads=(1, 5))


def test_a_zero_factor_in_the_middle_of_a_product_scan(G):
    for p in (0, 1, G - 1, G, G + 1, 2 * G + 2):
        jb = SC.sc_zero_factor(G, p)
        sc_check(jb)
        for exclusive in SC.MODES:
            want = SC.sc_expected(*jb, exclusive=exclusive)
            z = G + p
            assert all(v != 0 for v in want[:z]) and all(v != 0 for v in want[3 * G + 3:])      # the neighbours are untouched
            assert all(v == 0 for v in want[z + 1:3 * G + 3])
            assert (want[z] != 0) == exclusive                                                  # the exclusive row at the zero: the product before it


@pytest.mark.parametrize("op", SC.OPS)
def test_scalar_repeated_and_skipped_indices(G, op):
    for jb in SC.sc_gathers(op, G):
        sc_check(jb)
    jb = SC.sc_job(op, SC.shapes(G)["ragged"], seed=5)
    for exclusive in SC.MODES:
        assert (sc_run(jb, exclusive, 5) == sc_run(SC.with_arange(jb), exclusive, 5)).all()


def test_scalar_powers(G):
    x = [3, 0, 1, SC.L - 1, 2 ** 256 - 1] + SC.sc_operands(SC.PRODUCT, 3, 8)
    for t in (1, 2, G + 3):
        got = T.scalar_powers(None, SC.rows(x), t, threads=5)
        assert got.shape == (len(x), t, 32)
        assert SC.ints(got) == [pow(v, i, SC.L) for v in x for i in range(t)]
    assert T.scalar_powers(None, SC.rows(x), 0).shape == (len(x), 0, 32)


def test_point_single_segments_around_the_unit_edges(GP):
    for n in SC.single_lengths(GP):
        pt_check(SC.pt_job([n], seed=n))


def test_point_shapes(GP):
    for k, (name, lens) in enumerate(SC.shapes(GP).items()):
        pt_check(SC.pt_job(lens, seed=20 + k))


def test_point_long_segment_that_many_threads_cut(GP):
    pt_check(SC.pt_job([3, 20 * 64 + 11, 0, 70, 1], seed=4), threads=(1, 7, 40))
    pt_check(SC.pt_triples(900, [1, 880, 19]), threads=(1, 6))


def test_one_point_referenced_t_times_and_p_minus_p(GP):
    t = 2 * GP + 5
    off = SC.offsets([t])
    out, st = T.point_cumsum(None, off, SC.catalogue(), np.zeros(t, np.uint32), None, False, 5)         # B, B, B, ..: B, 2B, 3B, ..
    m = SC.multiples(range(1, t + 1))
    assert not st.any() and all((out[i] == m[i + 1]).all() for i in range(t))
    pidx, neg = np.zeros(t, np.uint32), (np.arange(t) % 2).astype(np.uint8)                             # B, -B, B, -B, ..: B, 0, B, 0, ..
    out, st = T.point_cumsum(None, off, SC.catalogue(), pidx, neg, False, 5)
    assert not st.any() and not out[1::2].any() and (out[0::2] == SC.catalogue()[0]).all()
    pidx = np.full(t, SC.IDENTITY_ROW, np.uint32)                                                       # identity operands
    pidx[GP] = 2
    out, st = T.point_cumsum(None, off, SC.catalogue(), pidx, None, False, 5)
    assert not st.any() and not out[:GP].any() and (out[GP:] == SC.catalogue()[2]).all()


def test_an_encoding_that_does_not_decode_at_the_front_middle_and_back(GP):
    lens = [GP + 3, 2 * GP + 6, 5]
    off = SC.offsets(lens)
    first, last = int(off[1]), int(off[2]) - 1
    for p in (first, first + GP, last):
        jb = SC.pt_job(lens, seed=p, bad_at=(p,))
        pt_check(jb, threads=(1, 5))
        for exclusive in SC.MODES:
            _, st = SC.pt_expected(*jb, exclusive=exclusive)
            lo = p + 1 if exclusive else p
            assert not st[:lo].any() and st[lo:last + 1].all() and not st[last + 1:].any()


def test_points_against_the_host_point_sum_on_the_prefix_segments(GP):
    """byte for byte against the existing point_sum over all prefixes (quadratic: a small job)"""
    lens = [0, 3, GP + 2, 0, 1, 7]
    off, pidx, neg = SC.pt_job(lens, seed=6, bad_at=(9,))
    pts = SC.catalogue()
    for exclusive in SC.MODES:
        p_off, p_idx, p_neg = [0], [], []
        for s in range(len(lens)):
            for t in range(int(off[s]), int(off[s + 1])):
                hi = t if exclusive else t + 1
                p_idx += list(pidx[int(off[s]):hi])
                p_neg += list(neg[int(off[s]):hi])
                p_off.append(len(p_idx))
        want, wst = T.point_sum(None, np.array(p_off, np.uint32), pts, np.array(p_idx, np.uint32), np.array(p_neg, np.uint8))
        out, st = T.point_cumsum(None, off, pts, pidx, neg, exclusive, 3)
        assert (st == wst).all() and (out == want).all()
    own = np.ascontiguousarray(pts[pidx])                                                               # pidx = None: term t is point t
    a, b = T.point_cumsum(None, off, own, None, neg), T.point_cumsum(None, off, pts, pidx, neg)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_argument_errors_write_nothing():
    op, off, a, _ = SC.sc_job(SC.SUM, [3, 0, 5], seed=4)
    a = SC.rows(a)
    idx = np.arange(8, dtype=np.uint32)
    out = np.full((8, 32), 0xEE, np.uint8)
    st = np.full(8, 0xEE, np.uint8)
    pts = np.ascontiguousarray(SC.catalogue()[:8])
    OF, A, IX, O, ST, P = (x.ctypes.data for x in (off, a, idx, out, st, pts))
    sc, pt = T.lib().zkp_scalar_scan_batch, T.lib().zkp_point_scan_batch
    for o in SC.OPS:
        for m in (0, 1):
            assert sc(None, o, m, 0, None, None, 0, None, 0, None) == 0                                 # n_seg = 0: a no-op
    for m in (0, 1):
        assert pt(None, m, 0, None, None, None, None, 0, 0, None, None) == 0
    empty = np.zeros(3, np.uint32)
    assert sc(None, 0, 0, 2, empty.ctypes.data, None, 0, None, 0, None) == 0                             # T = 0: a no-op
    assert pt(None, 0, 2, empty.ctypes.data, None, None, None, 0, 0, None, None) == 0
    assert sc(None, 0, 0, 0, OF, A, 8, None, 0, O) == 0 and pt(None, 0, 0, OF, None, None, P, 8, 0, O, ST) == 0    # n_seg = 0 with operands
    huge, one_idx = np.array([0, 2 ** 31], np.uint32), np.zeros(1, np.uint32)                            # more than 2^31 - 1 terms: refused before anything is read
    assert sc(None, 0, 0, 1, huge.ctypes.data, A, 8, one_idx.ctypes.data, 0, O) == BAD_STATEMENT
    assert pt(None, 0, 1, huge.ctypes.data, one_idx.ctypes.data, None, P, 8, 0, O, ST) == BAD_STATEMENT
    for o in (2, 3, -1):                                                                                # ZKP_SC_DOT has no scan; unknown ops
        assert sc(None, o, 0, 3, OF, A, 8, None, 0, O) == BAD_STATEMENT
    for m in (2, -1):
        assert sc(None, 0, m, 3, OF, A, 8, None, 0, O) == BAD_STATEMENT
        assert pt(None, m, 3, OF, None, None, P, 8, 0, O, ST) == BAD_STATEMENT
    one, dec = np.array([1, 3, 3, 8], np.uint32), np.array([0, 5, 3, 8], np.uint32)
    for bad in (one, dec):
        assert sc(None, 0, 0, 3, bad.ctypes.data, A, 8, None, 0, O) == BAD_STATEMENT
        assert pt(None, 0, 3, bad.ctypes.data, None, None, P, 8, 0, O, ST) == BAD_STATEMENT
    wild = idx.copy()
    wild[5] = 8
    assert sc(None, 0, 0, 3, OF, A, 8, wild.ctypes.data, 0, O) == BAD_STATEMENT                          # an index at the operand's length
    assert pt(None, 0, 3, OF, wild.ctypes.data, None, P, 8, 0, O, ST) == BAD_STATEMENT
    for n in (7, 9):                                                                                    # no index list: the operand must have T rows
        assert sc(None, 0, 0, 3, OF, A, n, None, 0, O) == BAD_STATEMENT
        assert pt(None, 0, 3, OF, None, None, P, n, 0, O, ST) == BAD_STATEMENT
    assert sc(None, 0, 0, 3, None, A, 8, None, 0, O) == BAD_STATEMENT                                    # NULL buffers
    assert sc(None, 0, 0, 3, OF, None, 8, None, 0, O) == BAD_STATEMENT
    assert sc(None, 0, 0, 3, OF, A, 8, None, 0, None) == BAD_STATEMENT
    assert pt(None, 0, 3, None, None, None, P, 8, 0, O, ST) == BAD_STATEMENT
    assert pt(None, 0, 3, OF, None, None, None, 8, 0, O, ST) == BAD_STATEMENT
    assert pt(None, 0, 3, OF, None, None, P, 8, 0, None, ST) == BAD_STATEMENT
    assert pt(None, 0, 3, OF, None, None, P, 8, 0, O, None) == BAD_STATEMENT
    assert (out == 0xEE).all() and (st == 0xEE).all()
    assert sc(None, 0, 0, 3, OF, A, 8, None, 0, O) == 0 and not (out == 0xEE).all(axis=1).any()          # (the same arguments, unbroken, are a call)
    out[:] = 0xEE
    assert pt(None, 0, 3, OF, None, None, P, 8, 0, O, ST) == 0 and not (st == 0xEE).any()


def test_threshold_setters_and_the_declarations_parse():
    from zkp_amd import cabi
    tb, dev = cabi.signatures("zkp_toolbox.h"), cabi.signatures("zkp_mi355x.h")
    assert {"zkp_scalar_scan_batch", "zkp_point_scan_batch", "zkp_toolbox_set_scalar_scan_min_terms", "zkp_toolbox_get_scalar_scan_min_terms",
            "zkp_toolbox_set_point_scan_min_terms", "zkp_toolbox_get_point_scan_min_terms"} <= set(tb)
    assert {"zkp_sc_scan", "zkp_sc_scan_dev", "zkp_sc_scan_group", "zkp_sc_scan_launches", "zkp_scan_points", "zkp_scan_points_dev", "zkp_scan_points_group",
            "zkp_scan_points_launches"} <= set(dev)
    assert len(dev["zkp_sc_scan"][1]) == 9 and len(dev["zkp_sc_scan_dev"][1]) == 10 and len(dev["zkp_scan_points"][1]) == 10
    assert len(dev["zkp_scan_points_dev"][1]) == 11 and len(tb["zkp_scalar_scan_batch"][1]) == 10 and len(tb["zkp_point_scan_batch"][1]) == 11
    for op in SC.OPS:
        old = T.get_scalar_scan_min_terms(op)
        try:
            for v in (77 + op, 0, 2 ** 64 - 1):
                T.set_scalar_scan_min_terms(op, v)
                assert T.get_scalar_scan_min_terms(op) == v
                assert all(T.get_scalar_scan_min_terms(o) != 77 + op for o in SC.OPS if o != op)
        finally:
            T.set_scalar_scan_min_terms(op, old)
    assert T.get_scalar_scan_min_terms(2) == 2 ** 64 - 1
    old = T.get_point_scan_min_terms()
    try:
        for v in (91, 0, 2 ** 64 - 1):
            T.set_point_scan_min_terms(v)
            assert T.get_point_scan_min_terms() == v
    finally:
        T.set_point_scan_min_terms(old)


def test_the_plan_functions(G, GP):
    from zkp_amd.engine import load_library
    lib = load_library()
    for fn, g in ((lib.zkp_sc_scan_launches, G), (lib.zkp_scan_points_launches, GP)):
        assert fn(0) == 0 and fn(1) == fn(g) and fn(g + 1) == fn(g) + 2
        edges = SC.launch_edges(fn)
        assert len(edges) >= 3 and [n for n, _ in edges] == [edges[0][0] + 2 * k for k in range(len(edges))]
        for n, t in edges[1:]:
            assert fn(t - 1) == n - 2 and fn(t) == n


@pytest.mark.parametrize("name,args,needle", [("feldman_vss_batch.py", ["5", "3", "6"], "30 of 30 shares verified"),
                                              ("running_tally_batch.py", ["3", "9"], "27 of 27 running totals decrypted")])
def test_the_examples_on_the_host(name, args, needle):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", name)] + args + ["--host"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert needle in r.stdout, r.stdout


@pytest.mark.parametrize("op", SC.OPS)
def test_the_host_scans_under_sanitizers(tmp_path_factory, op):
    """tests/host/scan_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: hostbk::sc_scan_n and
    hostbk::point_scan_n on a ragged job with index lists, on heap blocks of exactly the size a call may touch.  Exit 0, silent sanitizers, every
    printed row the expected one."""
    exe = _sanitized_program(tmp_path_factory)
    rng = np.random.default_rng(op)
    lens = [0, 0, 1, 2, 3, 0, 5, 1, 1, 7, 40, 0, 0, 2, 600, 1, 90, 0, 33, 64, 2, 1, 0, 47, 0, 0]
    off = SC.offsets(lens)
    t, n_a = int(off[-1]), 37
    a = SC.sc_operands(op, n_a, 7)
    a[3], a[36] = 2 ** 256 - 1, SC.L + 5
    aidx = rng.integers(0, n_a, size=t).astype(np.uint32)
    aidx[0], aidx[-1] = n_a - 1, n_a - 1                          # the last row, at both ends
    _, pidx, neg = SC.pt_job(lens, seed=op, bad_at=(int(off[14]) + 300,))
    pts = SC.catalogue()
    hexrows = lambda v: "\n".join(bytes(x).hex() for x in v)
    job = tmp_path_factory.mktemp("job") / ("job%d.txt" % op)
    job.write_text("%d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n%s\n" % (op, len(off) - 1, t, n_a, len(pts), " ".join(map(str, off)), " ".join(map(str, aidx)),
                                                                 " ".join(map(str, pidx)), " ".join(map(str, neg)), hexrows(SC.rows(a)), hexrows(pts)))
    r = subprocess.run([str(exe), str(job)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    for mode, exclusive in enumerate(SC.MODES):
        got = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("S%d " % mode)]
        assert [int.from_bytes(bytes.fromhex(h), "little") for h in got] == SC.sc_expected(op, off, a, aidx, exclusive)
        want, wst = SC.pt_expected(off, pidx, neg, exclusive)
        got = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("P%d " % mode)]
        assert [h for h, _ in got] == [bytes(x).hex() for x in want] and [int(s) for _, s in got] == wst.tolist()


_exe = {}


def _sanitized_program(tmp_path_factory):
    if "exe" not in _exe:
        gxx = shutil.which("g++")
        assert gxx, "g++ is needed (it builds the host library too)"
        exe = tmp_path_factory.mktemp("scan") / "scan_host_main"
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                        os.path.join(ROOT, "tests", "host", "scan_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                        "-o", str(exe)], check=True, capture_output=True, text=True)
        _exe["exe"] = exe
    return _exe["exe"]

"""Segmented scalar sums, products and dot products on the host backend (no GPU): toolbox.scalar_sum / scalar_product / scalar_dot with eng = None are
hostbk::sc_reduce_n, which cuts the TERM axis over its threads, so a long segment becomes per-thread partials combined at the end.  Every result is
compared with Python integers mod l (tests/scalar_reduce_cases.py) for 1, 5 and 40 threads and all three ops; then the same code runs in a
stand-alone program under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import scalar_reduce_cases as RC
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (1, 5, 40)
BAD_STATEMENT = -10


@pytest.fixture(scope="module")
def G():
    from zkp_amd.engine import load_library
    g = int(load_library().zkp_sc_reduce_group())           # pure arithmetic: no context, no GPU
    assert g >= 4
    return g


def run(jb, threads):
    op, off, a, aidx, b, bidx = jb
    return T.scalar_reduce(None, op, off, RC.rows(a), aidx, None if b is None else RC.rows(b), bidx, threads=threads)


def check(jb, threads=THREADS):
    want = RC.expected(*jb)
    for t in threads:
        assert RC.ints(run(jb, t)) == want, (jb[0], t)
    return want


@pytest.mark.parametrize("op", RC.OPS)
def test_single_segments_around_the_group_edges(G, op):
    for n in RC.single_lengths(G):
        want = check(RC.job(op, [n], seed=n))
        if n == 0:
            assert want == [1 if op == RC.PRODUCT else 0]


@pytest.mark.parametrize("op", RC.OPS)
def test_ragged_job_with_a_segment_that_five_threads_cut(G, op):
    lens = RC.ragged_lengths(G)
    jb = RC.job(op, lens, seed=2)
    total = int(jb[1][-1])
    assert 850 <= total <= 950 and max(lens) == 600 > total // 5 and lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1]
    want = check(jb)
    ident = 1 if op == RC.PRODUCT else 0
    assert all(want[i] == ident for i, n in enumerate(lens) if n == 0)


@pytest.mark.parametrize("op", RC.OPS)
def test_edge_values_at_the_first_last_and_group_edge_positions(G, op):
    for shift in range(0, len(RC.EDGES), 3):
        check(RC.edge_rotation(op, G, shift))


def test_all_rows_2_256_minus_1(G):
    n = G + 3
    big = [2 ** 256 - 1] * n
    off = RC.offsets([n])
    assert RC.ints(T.scalar_sum(None, off, RC.rows(big))) == [n * (2 ** 256 - 1) % RC.L]
    assert RC.ints(T.scalar_product(None, off, RC.rows(big))) == [pow(2 ** 256 - 1, n, RC.L)]
    assert RC.ints(T.scalar_dot(None, off, RC.rows(big), RC.rows(big))) == [n * (2 ** 256 - 1) ** 2 % RC.L]


def test_a_zero_factor_at_every_edge_position(G):
    for p in RC.positions(2 * G + 3, G):
        want = check(RC.product_with_zero_at(G, p))
        assert want[1] == 0 and want[0] != 0 and want[2] != 0


@pytest.mark.parametrize("op", RC.OPS)
def test_gathers_with_repeated_indices(G, op):
    jobs = RC.gathers(op, G)
    for jb in jobs:
        check(jb)
    if op == RC.PRODUCT:                                   # the last job is j^i for i = 0 .. G + 1
        _, off, base, aidx, _, _ = jobs[-1]
        assert RC.expected(*jobs[-1]) == [pow(base[2], i, RC.L) for i in range(G + 2)]


@pytest.mark.parametrize("op", RC.OPS)
def test_null_and_arange_indices_give_the_same_bytes(G, op):
    jb = RC.job(op, RC.ragged_lengths(G), seed=5)
    for t in THREADS:
        assert (run(jb, t) == run(RC.with_arange(jb), t)).all()


def test_argument_errors_write_nothing():
    op, off, a, _, b, _ = RC.job(RC.DOT, [3, 0, 5], seed=4)
    a, b = RC.rows(a), RC.rows(b)
    idx = np.arange(8, dtype=np.uint32)
    out = np.full((3, 32), 0xEE, np.uint8)
    OF, A, B, IX, O = (x.ctypes.data for x in (off, a, b, idx, out))
    call = T.lib().zkp_scalar_reduce_batch
    for o in RC.OPS:
        assert call(None, o, 0, None, None, 0, None, None, 0, None, 0, None) == 0                 # n_out = 0: a no-op
    for o in (3, -1):
        assert call(None, o, 3, OF, A, 8, None, None, 0, None, 0, O) == BAD_STATEMENT             # an unknown op
    for o in (RC.SUM, RC.PRODUCT):                                                                # b, n_b, bidx belong to DOT
        assert call(None, o, 3, OF, A, 8, None, B, 0, None, 0, O) == BAD_STATEMENT
        assert call(None, o, 3, OF, A, 8, None, None, 8, None, 0, O) == BAD_STATEMENT
        assert call(None, o, 3, OF, A, 8, None, None, 0, IX, 0, O) == BAD_STATEMENT
    one, dec = np.array([1, 3, 3, 8], np.uint32), np.array([0, 5, 3, 8], np.uint32)
    for bad in (one, dec):
        assert call(None, RC.SUM, 3, bad.ctypes.data, A, 8, None, None, 0, None, 0, O) == BAD_STATEMENT
    wild = idx.copy()
    wild[5] = 8
    assert call(None, RC.SUM, 3, OF, A, 8, wild.ctypes.data, None, 0, None, 0, O) == BAD_STATEMENT      # an index at the operand's length
    assert call(None, RC.DOT, 3, OF, A, 8, None, B, 8, wild.ctypes.data, 0, O) == BAD_STATEMENT
    assert call(None, RC.SUM, 3, OF, A, 7, None, None, 0, None, 0, O) == BAD_STATEMENT                  # no index list: n_a must be T
    assert call(None, RC.SUM, 3, OF, A, 9, None, None, 0, None, 0, O) == BAD_STATEMENT
    assert call(None, RC.DOT, 3, OF, A, 8, None, B, 7, None, 0, O) == BAD_STATEMENT
    assert call(None, RC.SUM, 3, None, A, 8, None, None, 0, None, 0, O) == BAD_STATEMENT                # NULL buffers
    assert call(None, RC.SUM, 3, OF, None, 8, None, None, 0, None, 0, O) == BAD_STATEMENT
    assert call(None, RC.DOT, 3, OF, A, 8, None, None, 8, None, 0, O) == BAD_STATEMENT
    assert call(None, RC.SUM, 3, OF, A, 8, None, None, 0, None, 0, None) == BAD_STATEMENT
    assert (out == 0xEE).all()
    assert call(None, RC.DOT, 3, OF, A, 8, None, B, 8, None, 0, O) == 0 and not (out == 0xEE).all()    # (the same arguments, unbroken, are a call)


def test_threshold_setter_and_the_declarations_parse():
    from zkp_amd import cabi
    tb, dev = cabi.signatures("zkp_toolbox.h"), cabi.signatures("zkp_mi355x.h")
    assert {"zkp_scalar_reduce_batch", "zkp_toolbox_set_scalar_reduce_min_terms", "zkp_toolbox_get_scalar_reduce_min_terms"} <= set(tb)
    assert {"zkp_sc_reduce", "zkp_sc_reduce_dev", "zkp_sc_reduce_group", "zkp_sc_reduce_levels"} <= set(dev)
    assert len(dev["zkp_sc_reduce"][1]) == 11 and len(dev["zkp_sc_reduce_dev"][1]) == 12 and len(tb["zkp_scalar_reduce_batch"][1]) == 12
    for op in RC.OPS:
        old = T.get_scalar_reduce_min_terms(op)
        try:
            for v in (77 + op, 0, 2 ** 64 - 1):
                T.set_scalar_reduce_min_terms(op, v)
                assert T.get_scalar_reduce_min_terms(op) == v
                assert all(T.get_scalar_reduce_min_terms(o) != 77 + op for o in RC.OPS if o != op)
        finally:
            T.set_scalar_reduce_min_terms(op, old)


def test_the_plan_functions(G):
    from zkp_amd.engine import load_library
    levels = load_library().zkp_sc_reduce_levels
    assert levels(0) == 0 and levels(1) == 1 and levels(G) == 1 and levels(G + 1) == 2
    edges = RC.level_edges(levels)
    assert [lv for lv, _ in edges] == list(range(1, len(edges) + 1))
    for lv, t in edges[1:]:
        assert levels(t - 1) == lv - 1 and levels(t) == lv


def test_the_threshold_elgamal_example_on_the_host():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "threshold_elgamal_batch.py"), "6", "3", "5", "--host"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "6 of 6 amounts decrypted" in r.stdout and "0 of 6 amounts decrypted" in r.stdout


@pytest.mark.parametrize("op", RC.OPS)
def test_sc_reduce_n_under_sanitizers(tmp_path_factory, op):
    """tests/host/scalar_reduce_host_main.cpp + host/host_backend.cpp, g++ -fsanitize=address,undefined, as a child process: hostbk::sc_reduce_n on a
    ragged job with index lists, on heap blocks of exactly the size a call may touch.  Exit 0, silent sanitizers, every printed scalar the integer."""
    exe = _sanitized_program(tmp_path_factory)
    rng = np.random.default_rng(op)
    lens = RC.ragged_lengths()
    off = RC.offsets(lens)
    t, n_a, n_b = int(off[-1]), 37, 41
    a, b = RC.operands(op, n_a, 7)
    b = None if b is None else b + RC.operands(op, n_b - n_a, 8)[0]
    a[3], a[36] = 2 ** 256 - 1, RC.L
    aidx = rng.integers(0, n_a, size=t).astype(np.uint32)
    bidx = rng.integers(0, n_b, size=t).astype(np.uint32) if op == RC.DOT else None
    aidx[0], aidx[-1] = n_a - 1, n_a - 1                       # the last row, at both ends
    want = RC.expected(op, off, a, aidx, b, bidx)
    hexrows = lambda v: "\n".join(int(x).to_bytes(32, "little").hex() for x in v)
    job = tmp_path_factory.mktemp("job") / ("job%d.txt" % op)
    job.write_text("%d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n" % (op, len(off) - 1, t, n_a, n_b if b is not None else 0, " ".join(map(str, off)), " ".join(map(str, aidx)),
                                                           "" if bidx is None else " ".join(map(str, bidx)), hexrows(a), "" if b is None else hexrows(b)))
    r = subprocess.run([str(exe), str(job)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")]
    assert [int.from_bytes(bytes.fromhex(h), "little") for _, h in lines] == want


_exe = {}


def _sanitized_program(tmp_path_factory):
    if "exe" not in _exe:
        gxx = shutil.which("g++")
        assert gxx, "g++ is needed (it builds the host library too)"
        exe = tmp_path_factory.mktemp("sc_reduce") / "scalar_reduce_host_main"
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                        os.path.join(ROOT, "tests", "host", "scalar_reduce_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "host_backend.cpp"),
                        "-o", str(exe)], check=True, capture_output=True, text=True)
        _exe["exe"] = exe
    return _exe["exe"]

"""Segmented scalar sums, products and dot products on the MI355X: zkp_sc_reduce / _dev (k_sc_fold, zkp_amd/csrc/sc_reduce.h) and the toolbox routing
in front of them.  Every result is compared with Python integers mod l (tests/scalar_reduce_cases.py) and, byte for byte, with the host backend on
the same job.  Lengths sit around the fold's group size G and around the smallest term counts with two and three levels, all read from the library
(zkp_sc_reduce_group, zkp_sc_reduce_levels) and never written here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import scalar_reduce_cases as RC
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -2
BAD_STATEMENT = -10
NEVER = 2 ** 64 - 1


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def G(eng):
    g = int(eng._lib.zkp_sc_reduce_group())
    assert g >= 4
    return g


@pytest.fixture(scope="module")
def edges(eng):
    """[(levels, smallest T)] for every level count a T <= 2^22 has"""
    e = RC.level_edges(eng._lib.zkp_sc_reduce_levels)
    assert len(e) >= 2 and e[0] == (1, 1)
    return e


@pytest.fixture()
def always_device():
    old = [T.get_scalar_reduce_min_terms(op) for op in RC.OPS]
    for op in RC.OPS:
        T.set_scalar_reduce_min_terms(op, 0)
    yield
    for op, v in zip(RC.OPS, old):
        T.set_scalar_reduce_min_terms(op, v)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def arrays(jb):
    op, off, a, aidx, b, bidx = jb
    return op, off, RC.rows(a), aidx, None if b is None else RC.rows(b), bidx


def check(eng, jb, toolbox=True):
    """Engine.scalar_reduce == the integers == the host backend's bytes (== the toolbox on the device route)"""
    want = RC.expected(*jb)
    op, off, a, aidx, b, bidx = arrays(jb)
    got = eng.scalar_reduce(op, off, a, aidx, b, bidx)
    assert RC.ints(got) == want
    assert (T.scalar_reduce(None, op, off, a, aidx, b, bidx, threads=5) == got).all()
    if toolbox:
        assert (T.scalar_reduce(eng, op, off, a, aidx, b, bidx) == got).all()
    return want


@pytest.mark.parametrize("op", RC.OPS)
def test_single_segments_around_the_group_edges(eng, G, always_device, op):
    for n in RC.single_lengths(G):
        want = check(eng, RC.job(op, [n], seed=n))
        if n == 0:
            assert want == [1 if op == RC.PRODUCT else 0]


@pytest.mark.parametrize("op", RC.OPS)
def test_ragged_job(eng, G, always_device, op):
    lens = RC.ragged_lengths(G)
    want = check(eng, RC.job(op, lens, seed=2))
    ident = 1 if op == RC.PRODUCT else 0
    assert all(want[i] == ident for i, n in enumerate(lens) if n == 0)


@pytest.mark.parametrize("op", RC.OPS)
def test_edge_values_at_the_first_last_and_group_edge_positions(eng, G, always_device, op):
    for shift in range(0, len(RC.EDGES), 3):
        check(eng, RC.edge_rotation(op, G, shift))


def test_all_rows_2_256_minus_1(eng, G):
    n = 2 * G + 3
    big = RC.rows([2 ** 256 - 1] * n)
    off = RC.offsets([n])
    assert RC.ints(eng.scalar_reduce(RC.SUM, off, big)) == [n * (2 ** 256 - 1) % RC.L]
    assert RC.ints(eng.scalar_reduce(RC.PRODUCT, off, big)) == [pow(2 ** 256 - 1, n, RC.L)]
    assert RC.ints(eng.scalar_reduce(RC.DOT, off, big, None, big)) == [n * (2 ** 256 - 1) ** 2 % RC.L]


def test_a_zero_factor_at_every_edge_position(eng, G, always_device):
    for p in RC.positions(2 * G + 3, G):
        want = check(eng, RC.product_with_zero_at(G, p))
        assert want[1] == 0 and want[0] != 0 and want[2] != 0


@pytest.mark.parametrize("op", RC.OPS)
def test_gathers_with_repeated_indices(eng, G, always_device, op):
    for jb in RC.gathers(op, G):
        check(eng, jb)


@pytest.mark.parametrize("op", RC.OPS)
def test_null_and_arange_indices_give_the_same_bytes(eng, G, op):
    jb = RC.job(op, RC.ragged_lengths(G), seed=5)
    op_, off, a, aidx, b, bidx = arrays(jb)
    _, _, _, ai, _, bi = RC.with_arange(jb)
    assert (eng.scalar_reduce(op, off, a, None, b, None) == eng.scalar_reduce(op, off, a, ai, b, bi)).all()
    if op == RC.DOT:                                       # one operand in order, the other gathered
        assert (eng.scalar_reduce(op, off, a, None, b, bi) == eng.scalar_reduce(op, off, a, ai, b, None)).all()


@pytest.mark.parametrize("op", RC.OPS)
def test_single_segments_around_the_level_edges(eng, edges, op):
    """T2 - 1, T2, T2 + 1 and T3 - 1, T3, T3 + 1: the number of kernels named equals zkp_sc_reduce_levels"""
    levels = eng._lib.zkp_sc_reduce_levels
    eng.set_profiling(True)
    try:
        for lv, t_edge in edges[1:]:
            for n in (t_edge - 1, t_edge, t_edge + 1):
                jb = RC.job(op, [n], seed=n)
                want = RC.expected(*jb)
                op_, off, a, aidx, b, bidx = arrays(jb)
                got = eng.scalar_reduce(op, off, a, aidx, b, bidx)
                names = eng.last_kernels()["scalars"]
                assert levels(n) == (lv - 1 if n < t_edge else lv) and len(names) == levels(n), (n, names)
                assert all(nm.startswith("k_sc_fold<") for nm in names) and [nm.partition("@")[2] for nm in names] == [""] + [str(k) for k in range(2, len(names) + 1)]
                assert RC.ints(got) == want, n
                assert (T.scalar_reduce(None, op, off, a, aidx, b, bidx, threads=5) == got).all()
    finally:
        eng.set_profiling(False)


@pytest.mark.parametrize("op", RC.OPS)
def test_a_long_segment_between_short_ones_across_group_edges_of_levels_1_and_2(eng, G, edges, always_device, op):
    """the long segment's boundaries on both sides of a group edge at level 1 (items = terms: multiples of G) and at level 2 (a group of level 2 holds
    the two items of G / 2 groups of level 1: multiples of G * G / 2)"""
    g2 = G * G // 2
    assert edges[-1][0] >= 3 and edges[2][1] == g2 + 1
    for start, end in ((G - 1, g2 + 1), (G + 1, g2 - 1), (G, g2), (3, g2 + G + 1)):
        lens = [2, start - 2, end - start, 1, G + 1, 4]
        check(eng, RC.job(op, lens, seed=start))


@pytest.mark.parametrize("op", RC.OPS)
def test_one_output_and_one_output_per_term(eng, G, always_device, op):
    t = 65 * G + 1
    check(eng, RC.job(op, [t], seed=3))
    check(eng, RC.job(op, [1] * t, seed=4))


@pytest.mark.parametrize("op", RC.OPS)
def test_dev_form_on_torch_buffers_on_a_side_stream(G, op):
    """out lands in rows 1 .. n of a larger zeroed buffer and its neighbours stay zero; an index out of range in one segment leaves every other output
    right; the call recorded into a graph and replayed twice with the inputs changed between the replays"""
    torch = _torch()
    from zkp_amd.engine import Engine
    jb = RC.with_arange(RC.job(op, RC.ragged_lengths(G) + [3 * G + 7], seed=6))
    want = RC.expected(*jb)
    _, off, a, aidx, b, bidx = arrays(jb)
    n_out, n_terms = len(off) - 1, int(off[-1])
    dev = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")      # noqa: E731
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_off, d_a, d_ai = dev(off), dev(a), dev(aidx)
    d_b, d_bi = (dev(b), dev(bidx)) if op == RC.DOT else (None, None)
    d_out = torch.zeros((n_out + 2, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ptr = lambda x: None if x is None else x.data_ptr()                                                 # noqa: E731
    n_b = len(b) if op == RC.DOT else 0

    def enqueue(ai, bi):
        e.scalar_reduce_dev(op, n_out, d_off.data_ptr(), d_a.data_ptr(), len(a), ptr(ai), ptr(d_b), n_b, ptr(bi), n_terms, d_out.data_ptr() + 32)

    try:
        for ai, bi in ((d_ai, d_bi), (None, None)):                      # gathered, then in order (n_a = n_terms)
            d_out.zero_()
            torch.cuda.synchronize()
            enqueue(ai, bi)
            e.synchronize()
            out = d_out.cpu().numpy()
            assert RC.ints(out[1:n_out + 1]) == want and not out[0].any() and not out[n_out + 1].any()
        # an index out of range: every output but the victim's is right, nothing outside out is touched
        victim = int(np.flatnonzero(np.diff(off.astype(np.int64)) == 600)[0])
        wild = aidx.copy()
        wild[int(off[victim]) + G + 1] = len(a) + 5
        d_wild = dev(wild)
        d_out.zero_()
        torch.cuda.synchronize()
        enqueue(d_wild, d_bi)
        e.synchronize()
        out = d_out.cpu().numpy()
        got = RC.ints(out[1:n_out + 1])
        assert [g for i, g in enumerate(got) if i != victim] == [w for i, w in enumerate(want) if i != victim]
        assert not out[0].any() and not out[n_out + 1].any()
        # misaligned pointers and a wrong operand length are refused before anything is queued
        d_out.zero_()
        torch.cuda.synchronize()
        lib, h = e._lib, e._h
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr(), d_a.data_ptr() + 8, len(a), d_ai.data_ptr(), ptr(d_b), n_b, ptr(d_bi), n_terms, d_out.data_ptr() + 32) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr(), d_a.data_ptr(), len(a), d_ai.data_ptr(), ptr(d_b), n_b, ptr(d_bi), n_terms, d_out.data_ptr() + 8) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr() + 2, d_a.data_ptr(), len(a), d_ai.data_ptr(), ptr(d_b), n_b, ptr(d_bi), n_terms, d_out.data_ptr() + 32) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr(), d_a.data_ptr(), len(a), d_ai.data_ptr() + 1, ptr(d_b), n_b, ptr(d_bi), n_terms, d_out.data_ptr() + 32) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr(), d_a.data_ptr(), len(a) - 1, None, ptr(d_b), n_b, ptr(d_bi), n_terms, d_out.data_ptr() + 32) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, n_out, d_off.data_ptr(), d_a.data_ptr(), len(a), d_ai.data_ptr(), ptr(d_b), n_b, ptr(d_bi), 2 ** 31, d_out.data_ptr() + 32) == ERR_ARG
        e.synchronize()
        assert not bool(d_out.any().item())
        # the graph: recorded (the same call has run above), then replayed over two other sets of inputs
        with e.capture() as cap:
            enqueue(d_ai, d_bi)
        assert not bool(d_out.any().item())                              # recorded, not run
        for seed in (21, 22):
            jb2 = RC.with_arange(RC.job(op, RC.ragged_lengths(G) + [3 * G + 7], seed=seed))
            _, _, a2, _, b2, _ = arrays(jb2)
            d_a.copy_(torch.from_numpy(a2))
            if op == RC.DOT:
                d_b.copy_(torch.from_numpy(b2))
            torch.cuda.synchronize()
            cap.graph.launch()
            e.synchronize()
            assert RC.ints(d_out.cpu().numpy()[1:n_out + 1]) == RC.expected(*jb2)
        cap.graph.close()
    finally:
        e.close()


@pytest.mark.parametrize("op", RC.OPS)
def test_results_do_not_depend_on_what_the_workspace_held(G, edges, op):
    from zkp_amd.engine import Engine
    jb = RC.job(op, [5, edges[-1][1] + 3, 0, 2 * G], seed=8)            # every level the plan has
    want = RC.expected(*jb)
    _, off, a, aidx, b, bidx = arrays(jb)
    e = Engine(0, test_hooks=True)
    try:
        for word in (0xFFFFFFFF, 3):
            e.debug_fill_workspace(8 << 20, word)
            assert RC.ints(e.scalar_reduce(op, off, a, aidx, b, bidx)) == want
    finally:
        e.close()


@pytest.mark.parametrize("op", RC.OPS)
def test_toolbox_routes_on_both_sides_of_the_threshold(eng, G, op):
    old = T.get_scalar_reduce_min_terms(op)
    thr = G + 9
    eng.set_profiling(True)
    try:
        T.set_scalar_reduce_min_terms(op, thr)
        for lens, device in (([3, thr - 5, 0, 1], False), ([3, thr - 5, 0, 2], True)):
            assert (sum(lens) >= thr) == device
            jb = RC.job(op, lens, seed=9)
            _, off, a, aidx, b, bidx = arrays(jb)
            eng.scalar_reduce(RC.SUM, RC.offsets([1]), RC.rows([5]))                   # (leaves one kernel name behind)
            assert len(eng.last_kernels()["scalars"]) == 1
            got = T.scalar_reduce(eng, op, off, a, aidx, b, bidx)
            assert RC.ints(got) == RC.expected(*jb)
            assert (len(eng.last_kernels()["scalars"]) == 2) == device                  # the device route ran two levels; the host route none
        T.set_scalar_reduce_min_terms(op, NEVER)
        eng.scalar_reduce(RC.SUM, RC.offsets([1]), RC.rows([5]))
        got = T.scalar_reduce(eng, op, off, a, aidx, b, bidx)
        assert RC.ints(got) == RC.expected(*jb) and len(eng.last_kernels()["scalars"]) == 1
    finally:
        T.set_scalar_reduce_min_terms(op, old)
        eng.set_profiling(False)


def test_timing_under_scalars(eng, edges):
    eng.set_profiling(True)
    try:
        jb = RC.job(RC.DOT, [edges[-1][1]], seed=1)
        _, off, a, aidx, b, bidx = arrays(jb)
        eng.scalar_reduce(RC.DOT, off, a, aidx, b, bidx)
        ms, total = eng.last_timing()
        assert ms["scalars"] > 0 and total >= ms["scalars"]
        assert len(eng.last_kernels()["scalars"]) == edges[-1][0]
    finally:
        eng.set_profiling(False)


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    _, off, a, _, b, _ = RC.job(RC.DOT, [3, 0, 5], seed=4)
    a, b = RC.rows(a), RC.rows(b)
    idx = np.arange(8, dtype=np.uint32)
    out = np.full((3, 32), 0xEE, np.uint8)
    OF, A, B, IX, O = (x.ctypes.data for x in (off, a, b, idx, out))
    for op in RC.OPS:
        assert lib.zkp_sc_reduce(h, op, 0, None, None, 0, None, None, 0, None, None) == 0
        assert lib.zkp_sc_reduce_dev(h, op, 0, None, None, 0, None, None, 0, None, 0, None) == 0
    assert lib.zkp_sc_reduce(None, RC.SUM, 3, OF, A, 8, None, None, 0, None, O) == ERR_ARG
    assert lib.zkp_sc_reduce_dev(None, RC.SUM, 3, OF, A, 8, None, None, 0, None, 8, O) == ERR_ARG
    for op in (3, -1):
        assert lib.zkp_sc_reduce(h, op, 3, OF, A, 8, None, None, 0, None, O) == ERR_ARG
        assert lib.zkp_sc_reduce_dev(h, op, 3, OF, A, 8, None, None, 0, None, 8, O) == ERR_ARG           # (rejected before any pointer is used)
        assert T.lib().zkp_scalar_reduce_batch(h, op, 3, OF, A, 8, None, None, 0, None, 0, O) == BAD_STATEMENT
    for op in (RC.SUM, RC.PRODUCT):
        for bargs in ((B, 0, None), (None, 8, None), (None, 0, IX)):
            assert lib.zkp_sc_reduce(h, op, 3, OF, A, 8, None, *bargs, O) == ERR_ARG
            assert lib.zkp_sc_reduce_dev(h, op, 3, OF, A, 8, None, *bargs, 8, O) == ERR_ARG
    one, dec = np.array([1, 3, 3, 8], np.uint32), np.array([0, 5, 3, 8], np.uint32)
    for bad in (one, dec):
        assert lib.zkp_sc_reduce(h, RC.SUM, 3, bad.ctypes.data, A, 8, None, None, 0, None, O) == ERR_ARG
        old = T.get_scalar_reduce_min_terms(RC.SUM)
        T.set_scalar_reduce_min_terms(RC.SUM, 0)
        try:
            assert T.lib().zkp_scalar_reduce_batch(h, RC.SUM, 3, bad.ctypes.data, A, 8, None, None, 0, None, 0, O) == BAD_STATEMENT
        finally:
            T.set_scalar_reduce_min_terms(RC.SUM, old)
    wild = idx.copy()
    wild[5] = 8
    assert lib.zkp_sc_reduce(h, RC.SUM, 3, OF, A, 8, wild.ctypes.data, None, 0, None, O) == ERR_ARG
    assert lib.zkp_sc_reduce(h, RC.DOT, 3, OF, A, 8, None, B, 8, wild.ctypes.data, O) == ERR_ARG
    assert lib.zkp_sc_reduce(h, RC.SUM, 3, OF, A, 7, None, None, 0, None, O) == ERR_ARG                   # no index list: n_a must be T
    assert lib.zkp_sc_reduce(h, RC.DOT, 3, OF, A, 8, None, B, 9, None, O) == ERR_ARG
    assert lib.zkp_sc_reduce(h, RC.SUM, 3, None, A, 8, None, None, 0, None, O) == ERR_ARG                 # NULL buffers
    assert lib.zkp_sc_reduce(h, RC.SUM, 3, OF, None, 8, None, None, 0, None, O) == ERR_ARG
    assert lib.zkp_sc_reduce(h, RC.DOT, 3, OF, A, 8, None, None, 8, None, O) == ERR_ARG
    assert lib.zkp_sc_reduce(h, RC.SUM, 3, OF, A, 8, None, None, 0, None, None) == ERR_ARG
    assert lib.zkp_sc_reduce_dev(h, RC.SUM, 3, OF, A, 8, None, None, 0, None, 8, None) == ERR_ARG
    assert lib.zkp_sc_reduce_dev(h, RC.SUM, 3, None, A, 8, None, None, 0, None, 8, O) == ERR_ARG
    assert (out == 0xEE).all()


def test_the_threshold_elgamal_example_on_the_engine():
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "threshold_elgamal_batch.py"), "256"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "256 of 256 amounts decrypted" in r.stdout and "0 of 256 amounts decrypted" in r.stdout

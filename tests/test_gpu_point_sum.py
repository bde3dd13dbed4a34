"""Batched RistrettoPoint sums on the MI355X: k_add_pairs behind zkp_add_points / _dev (two decodes, the complete addition and the encoder in one
launch) and the segmented fold behind zkp_sum_points / _dev (k_decode_affine, k_sum_fold level by level, k_sum_encode), with the toolbox routing in
front of them.  Checked byte for byte against the oracle (big-integer model for pairs, the C msm_many over a catalogue with net multiplicities for
sums), the host backend, and Engine.msm_many on the unit-scalar job callers built before, whose code is unchanged.  Sizes sit on the wavefront
and block edges; segment lengths sit around the fold's group size, which is read from zkp_sum_points_group() and never written here."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

from oracle import cbind as C
from tests import point_mul_cases as PC
from tests import point_sum_cases as SC
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_VARTIME

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096]
ERR_ARG = -2


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def group(eng):
    c = int(eng._lib.zkp_sum_points_group())
    assert c >= 4 and c % 2 == 0
    return c


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def pairs(op, n):
    a, b, _ = SC.pair_operands()
    want, st = SC.pair_expected(op)
    return tuple(PC.tiled(x, n) for x in (a, b, want, st))


def msm_route(eng, off, pidx, neg, points):
    """the route callers had before: Engine.msm_many with scalars 1 / l - 1"""
    t = int(off[-1])
    return eng.msm_many(off, SC.as_msm_job(off, pidx, neg), np.arange(t, dtype=np.uint32) if pidx is None else pidx, points, ZKP_VARTIME)


def check_sums(eng, off, pidx, neg, points, want, want_st, old_route=True):
    got, st = eng.sum_points(off, points, pidx, neg)
    assert (st == want_st).all()
    assert (got == want).all()
    host, host_st = T.point_sum(None, off, points, pidx, neg)
    assert (got == host).all() and (st == host_st).all()
    if old_route:
        old, old_st = msm_route(eng, off, pidx, neg, points)
        assert (got == old).all() and (st == old_st).all()
    return got, st


@pytest.mark.parametrize("op", [SC.ADD, SC.SUB])
@pytest.mark.parametrize("n", SIZES)
def test_pairs_equal_oracle_host_backend_and_msm_many(eng, n, op):
    a, b, want, want_st = pairs(op, n)
    assert want_st[0] == 1                                             # the smallest size holds an invalid operand
    if n >= 63:
        assert want_st.any() and not want_st.all()                     # invalid operands among valid ones
    got, st = eng.add_points(a, b, op)
    assert (st == want_st).all()
    assert (got == want).all()                                         # (the neighbours of an invalid operand included)
    assert not got[st == 1].any()
    host, host_st = (T.point_add if op == SC.ADD else T.point_sub)(None, a, b)
    assert (got == host).all() and (st == host_st).all()
    off = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    pts = np.ascontiguousarray(np.stack([a, b], axis=1).reshape(-1, 32))
    old, old_st = msm_route(eng, off, None, np.tile([0, op], n), pts)
    assert (got == old).all() and (st == old_st).all()


@pytest.mark.parametrize("sa,sb", list(itertools.product((0, 1), repeat=2)))
@pytest.mark.parametrize("op", [SC.ADD, SC.SUB])
def test_pair_strides_and_aliasing(eng, sa, sb, op):
    n = 257
    a, b, want, want_st = pairs(op, n)
    a0, b0 = int(np.flatnonzero(want_st == 0)[4]), int(np.flatnonzero(want_st == 0)[9])
    A = a if sa else a[a0:a0 + 1].copy()
    Bb = b if sb else b[b0:b0 + 1].copy()
    out, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    assert eng._lib.zkp_add_points(eng._h, n, A.ctypes.data, sa, Bb.ctypes.data, sb, op, out.ctypes.data, st.ctypes.data) == 0
    ref, ref_st = (T.point_add if op == SC.ADD else T.point_sub)(None, A if sa else np.repeat(A, n, axis=0), Bb if sb else np.repeat(Bb, n, axis=0))
    assert (out == ref).all() and (st == ref_st).all()
    if sa and sb:
        assert (out == want).all() and (st == want_st).all()
    if sa != sb:                                                       # the wrapper derives the strides from the shapes
        got, gst = eng.add_points(A if sa else A[0], Bb if sb else Bb[0], op)
        assert (got == out).all() and (gst == st).all()
    if not sb:                                                         # an invalid shared operand fails every output
        got, gst = eng.add_points(a, PC.enc_rows(SC.invalid_points()[3:4]), op)
        assert gst.all() and not got.any()
    if sa:                                                             # out may be a ...
        buf, st2 = a.copy(), np.zeros(n, np.uint8)
        assert eng._lib.zkp_add_points(eng._h, n, buf.ctypes.data, 1, Bb.ctypes.data, sb, op, buf.ctypes.data, st2.ctypes.data) == 0
        assert (buf == out).all() and (st2 == st).all()
    if sb:                                                             # ... or b
        buf, st2 = b.copy(), np.zeros(n, np.uint8)
        assert eng._lib.zkp_add_points(eng._h, n, A.ctypes.data, sa, buf.ctypes.data, 1, op, buf.ctypes.data, st2.ctypes.data) == 0
        assert (buf == out).all() and (st2 == st).all()


def test_special_pairs_need_no_special_case(eng):
    good = SC.valid_points()
    P = PC.tiled(PC.enc_rows(list(good)), 70)
    Z = np.zeros_like(P)
    negP, st = T.point_neg(eng, P)
    assert not st.any() and (negP == PC.tiled(PC.enc_rows([SC.negated(p) for p in good]), 70)).all()
    for got in (eng.add_points(P, negP), eng.add_points(P, P, SC.SUB), eng.add_points(Z, Z), eng.add_points(Z, Z, SC.SUB)):
        assert not got[0].any() and not got[1].any()                   # P - P, 0 + 0: the identity, status 0
    for got in (eng.add_points(P, Z), eng.add_points(Z, P), eng.add_points(P, Z, SC.SUB), T.point_neg(eng, negP)):
        assert (got[0] == P).all() and not got[1].any()
    dbl, _ = eng.add_points(P, P)
    two, _ = eng.mul_points(PC.rows([2]), P)
    assert (dbl == two).all()


@pytest.mark.parametrize("n", SIZES)
def test_sums_of_one_and_of_two_terms(eng, n):
    a, b, want, want_st = pairs(SC.ADD, n)
    # every segment one term: out == points where the row decodes
    bad_set = set(SC.invalid_points())
    bad_a = np.array([bytes(r) in bad_set for r in a])
    one = a.copy()
    one[bad_a] = 0
    off1 = np.arange(n + 1, dtype=np.uint32)
    got, st = eng.sum_points(off1, a)
    assert (got == one).all() and (st == bad_a).all()
    host, host_st = T.point_sum(None, off1, a)
    assert (got == host).all() and (st == host_st).all()
    # every segment two terms, added and subtracted
    off2 = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    pts = np.ascontiguousarray(np.stack([a, b], axis=1).reshape(-1, 32))
    check_sums(eng, off2, None, None, pts, want, want_st)
    wsub, wsub_st = (PC.tiled(x, n) for x in SC.pair_expected(SC.SUB))
    check_sums(eng, off2, None, np.tile([0, 1], n).astype(np.uint8), pts, wsub, wsub_st, old_route=n <= 257)


def test_ragged_job_with_and_without_indices(eng, group):
    pts, bad = SC.catalogue()
    off, pidx, neg, flagged = SC.ragged_job(group)
    lens = np.diff(off.astype(np.int64))
    assert {0, 1, 2, group - 1, group, group + 1, 2 * group, 2 * group + 1} <= set(lens.tolist())
    assert lens[0] == 0 and lens[1] == 0 and lens[-1] == 0             # empty segments first (doubled) and last
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    assert want_st.sum() == 1 and want_st[flagged] == 1 and 0 < off[flagged] % group < group - 2      # the bad point: one short sum inside a group
    assert not want[lens == 0].any()
    check_sums(eng, off, pidx, neg, pts, want, want_st)
    check_sums(eng, off, None, neg, np.ascontiguousarray(pts[pidx]), want, want_st)          # pidx == NULL: the same terms gathered
    want_add, want_add_st = SC.segments_expected(off, pidx, None, pts)
    check_sums(eng, off, pidx, None, pts, want_add, want_add_st)                             # neg == NULL
    # a bad point that no term references flags nothing
    keep = pidx != bad
    lens2 = np.array([int(keep[off[i]:off[i + 1]].sum()) for i in range(len(off) - 1)])
    off2 = np.concatenate([[0], np.cumsum(lens2)]).astype(np.uint32)
    w2, w2_st = SC.segments_expected(off2, pidx[keep], neg[keep], pts)
    assert not w2_st.any()
    check_sums(eng, off2, pidx[keep], neg[keep], pts, w2, w2_st)


def test_single_segments_run_plans_of_one_two_and_more_levels(eng, group):
    pts, _ = SC.catalogue()
    c = group
    seen = set()
    eng.set_profiling(True)
    try:
        for t in (c, c + 1, c * c // 2, c * c // 2 + 1, 2**17):
            off, pidx, neg = SC.single_segment(t)
            want, want_st = SC.segments_expected(off, pidx, neg, pts)
            got, st = eng.sum_points(off, pts, pidx, neg)
            names = eng.last_kernels()["reduce"]
            assert (got == want).all() and not st.any(), t
            assert len(names) == SC.plan_levels(t, c) and names[0] == "k_sum_fold<true>", (t, names)
            assert names[1:] == ["k_sum_fold<false>@%d" % k for k in range(2, len(names) + 1)]
            seen.add(len(names))
            ms = eng.last_timing()[0]
            assert ms["decode"] > 0 and ms["reduce"] > 0 and ms["combine"] > 0
            host, host_st = T.point_sum(None, off, pts, pidx, neg)
            assert (got == host).all() and not host_st.any()
            old, old_st = msm_route(eng, off, pidx, neg, pts)
            assert (got == old).all() and not old_st.any()
    finally:
        eng.set_profiling(False)
    assert {1, 2, 3} <= seen and max(seen) >= 4
    assert [SC.plan_levels(t, c) for t in (c, c + 1, c * c // 2, c * c // 2 + 1)] == [1, 2, 2, 3]


def test_a_long_segment_between_short_ones_and_known_sums(eng, group):
    pts, bad = SC.catalogue()
    t = 2**17
    _, pidx, neg = SC.single_segment(t + 5, seed=8)
    off = np.array([0, 3, 3 + t, 5 + t], np.uint32)                    # the carries of the long sum meet finished sums on both sides
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    check_sums(eng, off, pidx, neg, pts, want, want_st, old_route=False)
    pidx2 = pidx.copy()
    pidx2[3 + t // 2 + 7] = bad                                        # one bad term deep inside: the long sum alone is flagged
    got, st = eng.sum_points(off, pts, pidx2, neg)
    assert st.tolist() == [0, 1, 0] and not got[1].any() and (got[[0, 2]] == want[[0, 2]]).all()
    # k copies of P against k P from mul_points; P and -P alternating gives the identity
    P = pts[3:4]
    for k in (group * group + 3, 5000):
        got, st = eng.sum_points(np.array([0, k], np.uint32), P, np.zeros(k, np.uint32))
        kP, _ = eng.mul_points(PC.rows([k]), P)
        assert (got == kP).all() and not st.any()
        got, st = eng.sum_points(np.array([0, k - 1], np.uint32), P, np.zeros(k - 1, np.uint32), np.arange(k - 1) % 2)
        assert (not got.any() if (k - 1) % 2 == 0 else (got == P).all()) and not st.any()
    both = np.concatenate([P, PC.enc_rows([SC.negated(bytes(P[0]))])])
    got, st = eng.sum_points(np.array([0, 4096], np.uint32), both, (np.arange(4096) % 2).astype(np.uint32))
    assert not got.any() and not st.any()


def test_results_do_not_depend_on_what_the_workspace_held(group):
    from zkp_amd.engine import Engine
    pts, _ = SC.catalogue()
    t = group * group // 2 + 1                                         # three levels
    off, pidx, neg = SC.single_segment(t)
    off = np.array([0, 2, t - 1, t], np.uint32)
    want, want_st = SC.segments_expected(off, pidx, neg, pts)
    a, b, pw, pst = pairs(SC.SUB, 300)
    e = Engine(0, test_hooks=True)
    try:
        for word in (0xFFFFFFFF, 3):
            e.debug_fill_workspace(8 << 20, word)
            got, st = e.sum_points(off, pts, pidx, neg)
            assert (got == want).all() and (st == want_st).all()
            e.debug_fill_workspace(8 << 20, word)
            got, st = e.add_points(a, b, SC.SUB)
            assert (got == pw).all() and (st == pst).all()
    finally:
        e.close()


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    a, b, _, _ = pairs(SC.ADD, 70)
    a, b = a[66:70].copy(), b[66:70].copy()
    out, st = np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    A, Bp, O, ST = a.ctypes.data, b.ctypes.data, out.ctypes.data, st.ctypes.data
    assert lib.zkp_add_points(h, 0, None, 1, None, 1, 0, None, None) == 0 and lib.zkp_add_points_dev(h, 0, None, 0, None, 0, 1, None, None) == 0
    assert lib.zkp_sum_points(h, 0, None, None, None, None, 0, None, None) == 0
    assert lib.zkp_sum_points_dev(h, 0, None, None, None, None, 0, 0, None, None) == 0
    assert lib.zkp_add_points(None, 4, A, 1, Bp, 1, 0, O, ST) == ERR_ARG
    for args in ((None, 1, Bp, 1, 0, O, ST), (A, 1, None, 1, 0, O, ST), (A, 1, Bp, 1, 0, None, ST), (A, 1, Bp, 1, 0, O, None),
                 (A, 2, Bp, 1, 0, O, ST), (A, 1, Bp, 2, 1, O, ST), (A, 1, Bp, 1, 2, O, ST), (A, 1, Bp, 1, -1, O, ST)):
        assert lib.zkp_add_points(h, 4, *args) == ERR_ARG, args
        assert lib.zkp_add_points_dev(h, 4, *args) == ERR_ARG, args    # (rejected before any pointer is used)
    assert lib.zkp_add_points(h, 2**31, A, 0, Bp, 0, 0, O, ST) == ERR_ARG
    off, pidx, neg = np.arange(5, dtype=np.uint32), np.arange(4, dtype=np.uint32), np.zeros(4, np.uint8)
    OF, PI, NG = off.ctypes.data, pidx.ctypes.data, neg.ctypes.data
    assert lib.zkp_sum_points(None, 4, OF, PI, NG, A, 4, O, ST) == ERR_ARG
    assert lib.zkp_sum_points(h, 4, None, PI, NG, A, 4, O, ST) == ERR_ARG
    assert lib.zkp_sum_points(h, 4, OF, PI, NG, None, 4, O, ST) == ERR_ARG
    assert lib.zkp_sum_points(h, 4, OF, PI, NG, A, 4, None, ST) == ERR_ARG
    assert lib.zkp_sum_points(h, 4, OF, PI, NG, A, 4, O, None) == ERR_ARG
    assert lib.zkp_sum_points(h, 4, OF, PI, NG, A, 3, O, ST) == ERR_ARG                     # index 3 out of range
    assert lib.zkp_sum_points(h, 4, OF, None, NG, A, 3, O, ST) == ERR_ARG                   # no pidx: n_points must equal T
    assert lib.zkp_sum_points_dev(h, 4, OF, None, NG, A, 5, 4, O, ST) == ERR_ARG
    dec = np.array([0, 2, 1, 3, 4], np.uint32)
    assert lib.zkp_sum_points(h, 4, dec.ctypes.data, PI, NG, A, 4, O, ST) == ERR_ARG
    one = np.array([1, 1, 2, 3, 4], np.uint32)
    assert lib.zkp_sum_points(h, 4, one.ctypes.data, PI, NG, A, 4, O, ST) == ERR_ARG
    assert not out.any() and not st.any()
    # the toolbox reports the same as a bad statement, on the device route too
    assert T.lib().zkp_point_sum_batch(h, 4, OF, PI, NG, A, 3, 0, O, ST) == -10
    assert not out.any() and not st.any()


def test_toolbox_routes_on_both_sides_of_host_max_terms(eng, group):
    assert T.get_host_max_terms() == 0                                 # (the gpu fixture: every size goes to the device)
    a, b, want, want_st = pairs(SC.SUB, 65)
    pts, _ = SC.catalogue()
    off, pidx, neg, _ = SC.ragged_job(group, cycles=1)
    swant, swant_st = SC.segments_expected(off, pidx, neg, pts)
    eng.set_profiling(True)
    try:
        got, st = T.point_sub(eng, a, b)
        assert eng.last_kernels() == {"reduce": ["k_add_pairs"]}       # the device ran it
        assert (got == want).all() and (st == want_st).all()
        got, st = T.point_sum(eng, off, pts, pidx, neg)
        assert eng.last_kernels()["reduce"][0] == "k_sum_fold<true>"
        assert (got == swant).all() and (st == swant_st).all()
        # the other side of the threshold: the host threads, same bytes, no kernel
        T.set_host_max_terms(int(off[-1]))
        try:
            eng.add_points(a[:1], b[:1])                               # (leaves "k_add_pairs" as the last call's kernel)
            got, st = T.point_sum(eng, off, pts, pidx, neg)
            assert eng.last_kernels() == {"reduce": ["k_add_pairs"]}
            assert (got == swant).all() and (st == swant_st).all()
            got, st = T.point_sub(eng, a, b)
            assert (got == want).all() and (st == want_st).all()
            longer = np.concatenate([off, [off[-1] + 1]]).astype(np.uint32)            # one term more: the device again
            got, st = T.point_sum(eng, longer, pts, np.concatenate([pidx, [0]]).astype(np.uint32), np.concatenate([neg, [0]]).astype(np.uint8))
            assert eng.last_kernels()["reduce"][0] == "k_sum_fold<true>"
            assert (got[:-1] == swant).all() and (got[-1] == pts[0]).all()
        finally:
            T.set_host_max_terms(0)
    finally:
        eng.set_profiling(False)


def test_dev_forms_on_a_side_stream_and_recorded_into_a_graph(group):
    """zkp_add_points_dev in place followed by a zkp_sum_points_dev that reads its output, on torch device buffers and a side stream; then both
    recorded into one graph whose two replays follow new inputs placed in the same buffers.  An index out of range flags its sum."""
    torch = _torch()
    from zkp_amd.engine import Engine
    n = group * group + 76                                             # three levels
    lens = np.resize(np.array([0, 1, 2, group + 1, 5, 0, 3 * group, 7, 1]), 400)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n))]
    off = np.concatenate([[0], np.cumsum(lens), [n]]).astype(np.uint32)
    n_sums = len(off) - 1
    a, b, _, _ = pairs(SC.SUB, n)
    rng = np.random.default_rng(2)
    inputs = [(a, b), (a[::-1].copy(), b[rng.permutation(n)]), (b[rng.permutation(n)], a[::-1].copy())]
    plain = Engine(0)
    want = []
    for x, y in inputs:
        d, dst = plain.add_points(x, y, SC.SUB)
        s, sst = plain.sum_points(off, d)
        want.append((d, dst, s, sst))
    plain.close()
    assert want[0][1].any() and not want[0][3].any()                   # (a pair that fails leaves the identity: every row of d decodes)
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_a = torch.from_numpy(inputs[0][0]).to("cuda:0")
    d_b = torch.from_numpy(inputs[0][1]).to("cuda:0")
    d_off = torch.from_numpy(off.view(np.int32)).to("cuda:0")
    d_pst = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros((n_sums, 32), dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n_sums,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def enqueue():
        e.add_points_dev(n, d_a.data_ptr(), 1, d_b.data_ptr(), 1, SC.SUB, d_a.data_ptr(), d_pst.data_ptr())        # in place
        e.sum_points_dev(n_sums, d_off.data_ptr(), None, None, d_a.data_ptr(), n, n, d_out.data_ptr(), d_st.data_ptr())

    def check(k):
        d, dst, s, sst = want[k]
        assert (d_a.cpu().numpy() == d).all() and (d_pst.cpu().numpy() == dst).all()
        assert (d_out.cpu().numpy() == s).all() and (d_st.cpu().numpy() == sst).all()

    def load(k):
        d_a.copy_(torch.from_numpy(inputs[k][0]).to("cuda:0"))
        d_b.copy_(torch.from_numpy(inputs[k][1]).to("cuda:0"))
        d_out.zero_()
        d_st.zero_()
        torch.cuda.synchronize()

    enqueue()
    e.synchronize()
    check(0)
    # an index out of range on the device form flags that sum and no other
    pidx = np.arange(n, dtype=np.int32)
    victim = int(np.flatnonzero(lens > 1)[2])
    pidx[int(off[victim]) + 1] = n + 5
    d_pidx = torch.from_numpy(pidx).to("cuda:0")
    torch.cuda.synchronize()
    e.sum_points_dev(n_sums, d_off.data_ptr(), d_pidx.data_ptr(), None, d_a.data_ptr(), n, n, d_out.data_ptr(), d_st.data_ptr())
    e.synchronize()
    flagged = want[0][3].copy()
    flagged[victim] = 1
    expect = want[0][2].copy()
    expect[victim] = 0
    assert (d_st.cpu().numpy() == flagged).all() and (d_out.cpu().numpy() == expect).all()
    load(1)
    with e.capture() as cap:
        enqueue()
    assert not bool(d_out.any().item()) and bool((d_a.cpu() == torch.from_numpy(inputs[1][0])).all().item())          # recorded, not run
    cap.graph.launch()
    e.synchronize()
    check(1)
    load(2)
    cap.graph.launch()
    e.synchronize()
    check(2)
    cap.graph.close()
    e.close()


def test_the_elgamal_tally_example_on_the_engine(eng):
    spec = importlib.util.spec_from_file_location("elgamal_tally_batch", os.path.join(ROOT, "examples", "elgamal_tally_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 256
    r = mod.run(eng, n, key=bytes(range(1, 33)))
    assert r["accepted"] == n and r["rejected"] == n and r["decryption_verified"] and r["count"] == r["cast"]
    host = mod.run(None, n, key=bytes(range(1, 33)))                   # the same secrets on the host backend: the same bytes
    for k in ("C1", "C2", "D", "S1", "S2", "Z", "result"):
        assert (host[k] == r[k]).all(), k
    off = np.array([0, n, 2 * n], np.uint32)
    want, st = C.msm_many(off, SC.as_msm_job(off, None, None), np.arange(2 * n, dtype=np.uint32), np.concatenate([r["C1"], r["C2"]]), 0)
    assert not st.any() and (want[0] == r["S1"][0]).all() and (want[1] == r["S2"][0]).all()

"""Bounded discrete logarithms to a base of the caller's, unsigned and signed, on the MI355X: zkp_ctx_prepare_dlog_point (the base's fixed-base
table, k_dlog_setup, k_dlog_rows, the probe slots from the host) and zkp_dlog_point / _dev (k_dlog_prepare with or without the shift, then
k_dlog_steps slice by slice, outward from k = 0 when signed), with the toolbox routing in front of them.  The operands are those of
tests/dlog_point_cases.py: encode(k G) from the oracle for integers the test chose -- the expected output is k -- with rows that do not decode,
rows out of range and multiples of ANOTHER base between them.  The plan is read from the product and never written here."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import cbind as C
from tests import dlog_cases as DC
from tests import dlog_point_cases as PD
from tests import point_mul_cases as PC
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -2
SIGNED = 1


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plan(eng):
    lib = eng._lib
    group, chunk = int(lib.zkp_dlog_group()), int(lib.zkp_dlog_chunk())
    assert group >= 64 and chunk >= 2
    return group, chunk, (lambda n, signed=False: int((lib.zkp_dlog_slice_chunks_signed if signed else lib.zkp_dlog_slice_chunks)(n)))


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def slice_cases(name, bb, plan, signed):
    """the cases at a range wide enough for slice edges: (points, k, status, bits).  Unsigned: at least three launches; signed: four slices, so
    that the order z, z - 1, z + 1, 0 differs from the plain one everywhere.  The slice length depends on n, which does not depend on it."""
    group, chunk, slice_chunks = plan
    n = len(PD.operands(name, bb, 40, chunk, 1, signed)[0])
    for _ in range(4):                                                 # (a value met twice at one range and not at another changes n by a row or two)
        s = slice_chunks(n, signed)
        bits = bb + int(np.ceil(np.log2(2 * s * chunk))) + 1          # 2 S G m + m - 1 < 2^bits; signed: 2^bits = 4 S G m exactly
        pts, k, st = PD.operands(name, bb, bits, chunk, s, signed)
        if len(pts) == n:
            break
        n = len(pts)
    assert len(pts) == n and s == slice_chunks(n, signed)
    if signed:
        assert s & (s - 1) == 0 and (1 << bits) == 4 * s * chunk << bb
        assert int(k.min()) < -(s * chunk << bb) and int(k.max()) >= s * chunk << bb      # found rows in the first and in the last slice
    else:
        assert int(k.max()) >= 2 * s * chunk << bb
    return pts, k, st, bits


def check(e, slot, pts, bits, signed, want_k, want_st):
    k, st = e.dlog_point(slot, pts, bits, signed=signed)
    assert k.dtype == (np.int64 if signed else np.uint64)
    assert (st == want_st).all(), np.flatnonzero(st != want_st)
    assert (k == want_k).all(), np.flatnonzero(k != want_k)
    return k, st


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("bb", [4, 8])
@pytest.mark.parametrize("name", PD.BASES)
def test_the_cases_for_three_bases_in_both_modes(eng, plan, name, bb, signed):
    group, chunk, _ = plan
    eng.prepare_dlog_point(1, PD.base(name), bb)
    for bits in sorted({1, 2, bb - 1, bb, bb + 1, bb + 6, bb + 11}):
        pts, want_k, want_st = PD.operands(name, bb, bits, chunk, None, signed)
        assert (want_st == PD.FOUND).sum() >= 2 and (want_st == PD.INVALID).sum() >= 3 and (want_st == PD.NOT_FOUND).sum() >= 4
        check(eng, 1, pts, bits, signed, want_k, want_st)
    pts, want_k, want_st, bits = slice_cases(name, bb, plan, signed)      # chunk and slice edges, several launches
    k, st = check(eng, 1, pts, bits, signed, want_k, want_st)
    assert (PD.encode_multiples(name, k[st == PD.FOUND]) == pts[st == PD.FOUND]).all()


def test_a_slot_of_b_against_dlog_base_result_for_result(eng, plan):
    group, chunk, _ = plan
    for bb in (4, 8):
        eng.prepare_dlog(bb)
        eng.prepare_dlog_point(0, PC.BASEPOINT, bb)
        for bits in (1, bb, bb + 6, bb + 11):
            pts, want_k, want_st = DC.operands(bb, bits, chunk)
            k0, st0 = eng.dlog_base(pts, bits)
            k, st = eng.dlog_point(0, pts, bits)
            assert k.tobytes() == k0.tobytes() and st.tobytes() == st0.tobytes()
            assert (k == want_k).all() and (st == want_st).all()
    # every baby row of the slot is probed
    ks = np.arange(256)
    k, st = eng.dlog_point(0, DC.encode_multiples(ks), 8)
    assert not st.any() and (k == ks).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_wavefront_and_the_group(eng, plan, n):
    group, chunk, _ = plan
    eng.prepare_dlog_point(2, PD.base("H"), 8)
    for signed in (False, True):
        pts, want_k, want_st = PD.tiled("H", 8, 15, chunk, n, signed)
        check(eng, 2, pts, 15, signed, want_k, want_st)


def test_multiples_of_m_share_inversion_groups_to_base_h(eng, plan):
    """the zero case of dlog.h to another base: k' = j m makes the doubled candidate of step j the identity; in signed mode that is
    k = -2^(bits - 1) + j m.  Equal multiples of m put several zero factors into one shared inversion; found neighbours must not be harmed."""
    group, chunk, _ = plan
    bb = 8
    m = 1 << bb
    eng.prepare_dlog_point(2, PD.base("H"), bb)
    for signed in (False, True):
        for bits in (bb + chunk.bit_length() - 1, bb + chunk.bit_length() + 2):
            top, bias = 1 << (bits - bb), (1 << (bits - 1)) if signed else 0
            for j in (0, 3, chunk - 1, top // 2, top - 1):
                only = np.full(group + 3, j * m - bias)
                k, st = eng.dlog_point(2, PD.encode_multiples("H", only), bits, signed=signed)
                assert not st.any() and (k == only).all(), (signed, bits, j)
                mixed = np.array([j * m, j * m + 1, j * m, 5, j * m, j * m, (j + 1) * m - 1, j * m] * 40) - bias
                k, st = eng.dlog_point(2, PD.encode_multiples("H", mixed), bits, signed=signed)
                assert not st.any() and (k == mixed).all(), (signed, bits, j)
    junk = PC.enc_rows([PC.invalid_points()[0], PC.IDENTITY, PC.BASEPOINT, PC.IDENTITY, PC.IDENTITY, PC.invalid_points()[1]])
    for signed in (False, True):
        k, st = eng.dlog_point(2, junk, 13, signed=signed)
        assert st.tolist() == [1, 0, 2, 0, 0, 1] and not k.any()


def test_two_slots_used_alternately_leave_the_contexts_own_tables_alone(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    e = Engine(0)
    try:
        reg = PC.enc_rows(list(PC.hashed_points()))
        e.prepare_fixed_points(reg)
        e.prepare_dlog(6)
        b_pts, b_k, b_st = DC.operands(6, 13, chunk)
        mul_want = e.mul_base(PC.rows([5, 77]))
        e.prepare_dlog_point(3, PD.base("H"), 5)
        e.prepare_dlog_point(6, PD.base("G7"), 9)
        assert e.dlog_baby_bits == 6
        for rnd in range(3):
            for slot, name, bb in ((3, "H", 5), (6, "G7", 9)):
                for signed in (False, True):
                    pts, want_k, want_st = PD.operands(name, bb, 14, chunk, None, signed)
                    check(e, slot, pts, 14, signed, want_k, want_st)
            k, st = e.dlog_base(b_pts, 13)                            # the context's own B table in between
            assert (k == b_k).all() and (st == b_st).all() and e.dlog_baby_bits == 6
            assert (e.mul_base(PC.rows([5, 77])) == mul_want).all()
        slots = e.dlog_point_slots()
        assert [bb for _, bb in slots] == [0, 0, 0, 5, 0, 0, 9, 0]
        assert slots[3][0] == PD.base("H") and slots[6][0] == PD.base("G7") and slots[0][0] is None
        # the registry of prepare_fixed_points still answers: a product over registered points equals the oracle's
        sc = PC.rows([3] * len(reg))
        got, st = T.point_mul(e, sc, reg, 0)
        want, wst = T.point_mul(None, sc, reg, 0)
        assert (got == want).all() and not st.any()
    finally:
        e.close()


def test_replace_release_and_prepare_again(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    lib = None
    e = Engine(0)
    try:
        lib, h = e._lib, e._h
        H, G7 = PD.base("H"), PD.base("G7")
        Hrow = PC.enc_rows([H])
        assert lib.zkp_dlog_point_find(h, Hrow.ctypes.data) == -1 and lib.zkp_dlog_point_baby_bits(h, 4) == 0 and lib.zkp_dlog_point_last_use(h, 4) == 0
        e.prepare_dlog_point(4, H, 6)
        assert lib.zkp_dlog_point_find(h, Hrow.ctypes.data) == 4 and lib.zkp_dlog_point_baby_bits(h, 4) == 6
        got = np.zeros(32, np.uint8)
        assert lib.zkp_dlog_point_base(h, 4, got.ctypes.data) == 0 and got.tobytes() == H
        used = lib.zkp_dlog_point_last_use(h, 4)
        assert used > 0
        e.prepare_dlog_point(4, H, 6)                                  # the same again: a no-op that counts as a use
        assert lib.zkp_dlog_point_last_use(h, 4) > used
        pts, want_k, want_st = PD.operands("H", 6, 12, chunk, None, True)
        check(e, 4, pts, 12, True, want_k, want_st)
        e.prepare_dlog_point(4, H, 9)                                  # another size
        assert e.dlog_point_slots()[4] == (H, 9)
        check(e, 4, pts, 12, True, want_k, want_st)
        e.prepare_dlog_point(4, G7, 9)                                 # another base
        assert e.dlog_point_slots()[4] == (G7, 9) and lib.zkp_dlog_point_find(h, Hrow.ctypes.data) == -1
        g_pts, g_k, g_st = PD.operands("G7", 9, 12, chunk, None, True)
        check(e, 4, g_pts, 12, True, g_k, g_st)
        k, st = e.dlog_point(4, PD.encode_multiples("H", [1, 2]), 12)  # multiples of the base that left have no logarithm now
        assert st.tolist() == [2, 2] and not k.any()
        e.release_dlog_point(4)
        e.release_dlog_point(4)                                        # (an empty slot: a no-op)
        assert e.dlog_point_slots()[4] == (None, 0) and lib.zkp_dlog_point_base(h, 4, got.ctypes.data) == ERR_ARG
        out, st = np.full(2, 77, np.uint64), np.full(2, 9, np.uint8)
        assert lib.zkp_dlog_point(h, 4, 2, pts.ctypes.data, 12, 0, out.ctypes.data, st.ctypes.data) == ERR_ARG      # an empty slot: no default base
        assert (out == 77).all() and (st == 9).all()
        e.prepare_dlog_point(4, H, 4)
        check(e, 4, pts, 12, True, want_k, want_st)
    finally:
        e.close()


def test_results_do_not_depend_on_what_the_workspace_held(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    e = Engine(0, test_hooks=True)
    try:
        e.prepare_dlog_point(7, PD.base("H"), 8)
        for word in (0xFFFFFFFF, 2, 0):
            for signed in (False, True):
                pts, want_k, want_st = PD.operands("H", 8, 14, chunk, None, signed)
                e.debug_fill_workspace(8 << 20, word)
                check(e, 7, pts, 14, signed, want_k, want_st)
    finally:
        e.close()


def test_argument_errors_write_nothing_and_leave_the_slot_as_it_was(eng):
    lib, h = eng._lib, eng._h
    H = PD.base("H")
    eng.prepare_dlog_point(5, H, 8)
    Hrow = PC.enc_rows([H])
    pts = PD.encode_multiples("H", [3, 4])
    out, st = np.full(2, 77, np.uint64), np.full(2, 9, np.uint8)
    P, O, ST = pts.ctypes.data, out.ctypes.data, st.ctypes.data
    assert lib.zkp_dlog_point(h, 5, 0, None, 8, 0, None, None) == 0 and lib.zkp_dlog_point_dev(h, 5, 0, None, 8, SIGNED, None, None) == 0
    assert lib.zkp_dlog_point(None, 5, 2, P, 8, 0, O, ST) == ERR_ARG and lib.zkp_dlog_point_dev(None, 5, 2, P, 8, 0, O, ST) == ERR_ARG
    for args in ((None, 8, 0, O, ST), (P, 8, 0, None, ST), (P, 8, 0, O, None), (P, 0, 0, O, ST), (P, 49, SIGNED, O, ST), (P, 2**32 - 1, 0, O, ST),
                 (P, 8, 2, O, ST), (P, 8, 3, O, ST), (P, 8, -1, O, ST)):
        assert lib.zkp_dlog_point(h, 5, 2, *args) == ERR_ARG, args
        assert lib.zkp_dlog_point_dev(h, 5, 2, *args) == ERR_ARG, args  # (rejected before any pointer is used)
    assert lib.zkp_dlog_point(h, 5, 2**31, P, 8, 0, O, ST) == ERR_ARG
    for slot in (8, 9, 2**32 - 1):
        assert lib.zkp_dlog_point(h, slot, 2, P, 8, 0, O, ST) == ERR_ARG
        assert lib.zkp_ctx_prepare_dlog_point(h, slot, Hrow.ctypes.data, 8) == ERR_ARG and lib.zkp_ctx_release_dlog_point(h, slot) == ERR_ARG
        assert lib.zkp_dlog_point_baby_bits(h, slot) == 0
    empty = next(s for s, (_, bb) in enumerate(eng.dlog_point_slots()) if bb == 0 and s != 5)
    assert lib.zkp_dlog_point(h, empty, 2, P, 8, 0, O, ST) == ERR_ARG and lib.zkp_dlog_point_dev(h, empty, 2, P, 8, 0, O, ST) == ERR_ARG
    assert (out == 77).all() and (st == 9).all()
    # prepare: sizes, a NULL pointer, the identity and a base that does not decode leave the slot as it was
    for bad in (0, 3, 23, 2**31):
        assert lib.zkp_ctx_prepare_dlog_point(h, 5, Hrow.ctypes.data, bad) == ERR_ARG
    assert lib.zkp_ctx_prepare_dlog_point(h, 5, None, 8) == ERR_ARG and lib.zkp_ctx_prepare_dlog_point(None, 5, Hrow.ctypes.data, 8) == ERR_ARG
    assert lib.zkp_ctx_prepare_dlog_point(h, 5, np.zeros(32, np.uint8).ctypes.data, 8) == ERR_ARG
    for enc in PC.invalid_points()[:3]:
        assert lib.zkp_ctx_prepare_dlog_point(h, 5, PC.enc_rows([enc]).ctypes.data, 8) == ERR_ARG
        assert lib.zkp_ctx_prepare_dlog_point(h, empty, PC.enc_rows([enc]).ctypes.data, 8) == ERR_ARG
    assert lib.zkp_dlog_point_baby_bits(None, 5) == 0 and lib.zkp_dlog_point_find(None, Hrow.ctypes.data) == -1 and lib.zkp_dlog_point_find(h, None) == -1
    # a plan of more launches than the call accepts is refused before anything runs
    eng.prepare_dlog_point(5, H, 4)
    assert lib.zkp_dlog_point(h, 5, 2**31 - 1, P, 48, SIGNED, O, ST) == ERR_ARG
    assert (out == 77).all() and (st == 9).all()
    eng.prepare_dlog_point(5, H, 8)
    with eng.capture():
        assert lib.zkp_ctx_prepare_dlog_point(h, 5, Hrow.ctypes.data, 9) == ERR_ARG       # synchronous: not inside a capture
        assert lib.zkp_ctx_release_dlog_point(h, 5) == ERR_ARG
    assert eng.dlog_point_slots()[5] == (H, 8) and eng.dlog_point_slots()[empty] == (None, 0)
    k, s = eng.dlog_point(5, pts, 8, signed=True)
    assert k.tolist() == [3, 4] and not s.any()
    assert T.lib().zkp_point_dlog_batch(h, Hrow.ctypes.data, 2, P, 49, 0, O, ST, 0) == -10
    assert T.lib().zkp_point_dlog_batch(h, np.zeros(32, np.uint8).ctypes.data, 2, P, 8, 0, O, ST, 0) == -10
    steps = T.get_dlog_host_max_steps()
    T.set_dlog_host_max_steps(0)
    try:
        assert T.lib().zkp_point_dlog_batch(h, PC.enc_rows(PC.invalid_points()[:1]).ctypes.data, 2, P, 8, 0, O, ST, 0) == -11      # on the device route too
    finally:
        T.set_dlog_host_max_steps(steps)
    assert (out == 77).all() and (st == 9).all()


def test_toolbox_routes_on_both_sides_of_the_threshold_and_agrees_with_the_host(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    bb, bits = 8, 13
    host_bb, steps = T.get_dlog_baby_bits(), T.get_dlog_host_max_steps()
    T.set_dlog_baby_bits(bb)
    e = Engine(0)
    e.set_profiling(True)
    H = PD.base("H")
    dev = {True: {"decode": ["k_dlog_prepare<shift>"], "terms": ["k_dlog_steps"]}, False: {"decode": ["k_dlog_prepare"], "terms": ["k_dlog_steps"]}}
    marker = {"terms": ["k_mul_base"]}
    try:
        for signed in (False, True):
            pts, want_k, want_st = PD.operands("H", bb, bits, chunk, None, signed)
            n = len(pts)
            work = n * ((1 << (bits - bb)) + 128)                      # the call's host work in giant steps; the rule is per thread
            host_k, host_st = T.point_dlog(None, H, pts, bits, signed=signed)
            T.set_dlog_host_max_steps(work - 1)
            k, st = T.point_dlog(e, H, pts, bits, signed=signed, threads=1)
            assert e.last_kernels() == dev[signed]                     # the device ran it ...
            assert host_k.tobytes() == k.tobytes() and host_st.tobytes() == st.tobytes()
            assert (k == want_k).all() and (st == want_st).all()
            slot = e._lib.zkp_dlog_point_find(e._h, PC.enc_rows([H]).ctypes.data)
            assert slot >= 0 and e.dlog_point_slots()[slot] == (H, 16)  # ... on a slot the base got, of the default size
            e.mul_base(PC.rows([5]))                                   # (leaves "k_mul_base" as the last call's kernel)
            T.set_dlog_host_max_steps(work)
            k, st = T.point_dlog(e, H, pts, bits, signed=signed, threads=1)
            assert e.last_kernels() == marker                          # the host threads, no kernel
            assert (k == want_k).all() and (st == want_st).all()
            k, st = T.point_dlog(e, H, np.concatenate([pts, pts[:1]]), bits, signed=signed, threads=1)     # one point more: the device again
            assert e.last_kernels() == dev[signed]
            assert (k[:-1] == want_k).all() and k[-1] == want_k[0]
        # a caller who wants another size prepares the slot first: the call keeps it
        e.prepare_dlog_point(slot, H, 6)
        T.set_dlog_host_max_steps(0)
        k, st = T.point_dlog(e, H, pts, bits, signed=True)
        assert (k == want_k).all() and e.dlog_point_slots()[slot] == (H, 6)
        # eight slots: seven more bases fill them, a ninth base replaces the least recently used one
        e.prepare_dlog_point(slot, H, 4)
        others = PD.other_bases(8)
        ks = [0, 1, -1, 100, -255]
        for i, b in enumerate(others[:7]):
            k, st = T.point_dlog(e, b, DC.encode_multiples([(x * (100 + i)) % PD.L for x in ks]), 9, signed=True)
            assert not st.any() and k.tolist() == ks
        held = [s[0] for s in e.dlog_point_slots()]
        assert set(held) == {H} | set(others[:7])
        k, st = T.point_dlog(e, H, PD.encode_multiples("H", ks), 9, signed=True)       # H is used again: the first of the others is the oldest now
        assert not st.any() and k.tolist() == ks
        k, st = T.point_dlog(e, others[7], DC.encode_multiples([(x * 107) % PD.L for x in ks]), 9, signed=True)
        assert not st.any() and k.tolist() == ks
        held = [s[0] for s in e.dlog_point_slots()]
        assert set(held) == {H, others[7]} | set(others[1:7]) and e.dlog_point_slots()[slot] == (H, 4)
    finally:
        e.set_profiling(False)
        e.close()
        T.set_dlog_baby_bits(host_bb)
        T.set_dlog_host_max_steps(steps)


def test_dev_form_on_a_side_stream_and_recorded_into_a_graph_in_signed_mode(plan):
    """zkp_dlog_point_dev on torch device buffers and a side stream; then recorded into a graph (after one plain call, which builds the
    workspace) whose two replays follow new inputs placed in the same buffers.  Signed, four slices: the shift point's kernel, the prepare step
    and the launches, out of ascending order, follow each other inside the recording -- a plain chain with no parallel branches.  A graph
    recorded over a slot that was replaced since is refused."""
    torch = _torch()
    from zkp_amd.engine import Engine, ZkpError
    group, chunk, slice_chunks = plan
    bb = 6
    pts, want_k, want_st, bits = slice_cases("H", bb, plan, True)
    n = len(pts)
    rng = np.random.default_rng(5)
    perms = [np.arange(n), rng.permutation(n), rng.permutation(n)]
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    with e.capture():                                                  # an empty slot: the call cannot be recorded
        assert e._lib.zkp_dlog_point_dev(e._h, 0, n, 256, bits, SIGNED, 256, 256) == ERR_ARG
    e.prepare_dlog_point(0, PD.base("H"), bb)
    d_pts = torch.from_numpy(pts).to("cuda:0")
    d_out = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def enqueue():
        e.dlog_point_dev(0, n, d_pts.data_ptr(), bits, d_out.data_ptr(), d_st.data_ptr(), signed=True)

    def check_dev(p):
        assert (d_out.cpu().numpy() == want_k[p]).all() and (d_st.cpu().numpy() == want_st[p]).all()

    def load(p):
        d_pts.copy_(torch.from_numpy(pts[p]).to("cuda:0"))
        d_out.fill_(-1)
        d_st.fill_(7)
        torch.cuda.synchronize()

    enqueue()
    e.synchronize()
    check_dev(perms[0])
    load(perms[1])
    with e.capture() as cap:
        enqueue()
    assert bool((d_st == 7).all().item())                              # recorded, not run
    cap.graph.launch()
    e.synchronize()
    check_dev(perms[1])
    load(perms[2])
    cap.graph.launch()
    e.synchronize()
    check_dev(perms[2])
    e.prepare_dlog_point(0, PD.base("H"), bb + 1)                      # the slot is replaced: the recording points at freed rows
    with pytest.raises(ZkpError):
        cap.graph.launch()
    cap.graph.close()
    e.close()


def test_the_net_balances_example_on_the_engine(eng):
    spec = importlib.util.spec_from_file_location("net_balances_batch", os.path.join(ROOT, "examples", "net_balances_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, bits = 256, 24
    half = 1 << (bits - 1)
    rng = np.random.default_rng(9)
    transfers = rng.integers(-(half // 4), half // 4, size=(n, 3))
    transfers[:4] = [[0, 0, 0], [1, -2, 0], [half - 1, 0, 0], [-half, 0, 0]]
    transfers[4] = [half, 0, 0]                                        # out of range
    steps = T.get_dlog_host_max_steps()
    try:
        r = mod.run(eng, n, bits, key=bytes(range(1, 33)), transfers=transfers)
        assert r["accepted"] == n and r["rejected"] == n and r["match"]
        assert r["status"][4] == 2 and (np.delete(r["status"], 4) == 0).all()
        assert (np.delete(r["recovered"], 4) == np.delete(transfers.sum(axis=1), 4)).all()
        H = bytes(r["H"][0])
        assert eng._lib.zkp_dlog_point_find(eng._h, r["H"].ctypes.data) >= 0      # 256 accounts at 24 bits: the device route, on a slot of H
        small = [[5, -5, 0], [100, -300, 1], [2047, 0, 0], [1024, 1024, 0]] * 4
        host = mod.run(None, 16, 12, key=bytes(range(1, 33)), transfers=small)   # the same secrets on the host backend
        T.set_dlog_host_max_steps(0)
        again = mod.run(eng, 16, 12, key=bytes(range(1, 33)), transfers=small)
        for k in ("H", "C1", "C2", "Z", "sH", "recovered", "status"):
            assert (host[k] == again[k]).all(), k
        assert bytes(host["H"][0]) == H
    finally:
        T.set_dlog_host_max_steps(steps)

"""Bounded discrete logarithms to the basepoint on the MI355X: zkp_ctx_prepare_dlog (k_dlog_setup, k_dlog_rows, the probe slots from the host) and
zkp_dlog_base / _dev (k_dlog_prepare, then k_dlog_steps slice by slice), with the toolbox routing in front of them.  The operands are those of
tests/dlog_cases.py: encode(k B) from the oracle for integers the test chose -- the expected output is k -- with rows that do not decode and rows
without a logarithm in range between them.  The k values sit on the edges of the plan (baby table, chunk, slice, range), which is read from
zkp_dlog_group / _chunk / _slice_chunks and never written here."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import cbind as C
from tests import dlog_cases as DC
from tests import point_mul_cases as PC
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -2


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
    return group, chunk, (lambda n: int(lib.zkp_dlog_slice_chunks(n)))


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def slice_cases(bb, plan):
    """the cases at a range wide enough for slice edges: (points, k, status, bits); the slice length depends on n, which does not depend on it"""
    group, chunk, slice_chunks = plan
    n = len(DC.operands(bb, 40, chunk, 1)[0])
    s = slice_chunks(n)
    bits = bb + int(np.ceil(np.log2(2 * s * chunk))) + 1              # 2 S G m + m - 1 < 2^bits: at least three launches
    pts, k, st = DC.operands(bb, bits, chunk, s)
    assert len(pts) == n and int(k.max()) >= 2 * s * chunk << bb
    return pts, k, st, bits


def check(e, pts, bits, want_k, want_st):
    k, st = e.dlog_base(pts, bits)
    assert (st == want_st).all(), np.flatnonzero(st != want_st)
    assert (k == want_k).all(), np.flatnonzero(k != want_k)
    return k, st


@pytest.mark.parametrize("bb", [4, 8, 12])
def test_the_cases_at_three_table_sizes(eng, plan, bb):
    group, chunk, _ = plan
    eng.prepare_dlog(bb)
    assert eng.dlog_baby_bits == bb
    for bits in sorted({1, bb - 1, bb, bb + 1, bb + 6, bb + 11}):
        pts, want_k, want_st = DC.operands(bb, bits, chunk)
        assert (want_st == DC.FOUND).sum() >= 2 and (want_st == DC.INVALID).sum() >= 3 and (want_st == DC.NOT_FOUND).sum() >= 4
        check(eng, pts, bits, want_k, want_st)
    pts, want_k, want_st, bits = slice_cases(bb, plan)                 # chunk and slice edges, several launches
    k, st = check(eng, pts, bits, want_k, want_st)
    assert (DC.encode_multiples(k[st == DC.FOUND]) == pts[st == DC.FOUND]).all()


def test_the_baby_rows_are_the_oracles_encodings(eng):
    """every baby row is probed: k = 0 .. m - 1 found at bits = baby_bits, none of them at a giant step"""
    eng.prepare_dlog(8)
    ks = np.arange(256)
    k, st = eng.dlog_base(DC.encode_multiples(ks), 8)
    assert not st.any() and (k == ks).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_wavefront_and_the_group(eng, plan, n):
    group, chunk, _ = plan
    eng.prepare_dlog(8)
    pts, want_k, want_st = DC.tiled(8, 15, chunk, n)
    check(eng, pts, 15, want_k, want_st)


def test_multiples_of_m_share_inversion_groups(eng, plan):
    """the zero case: k = j m makes the doubled candidate of step j the identity.  With one chunk per point (2^bits = chunk m) the lanes of a
    workgroup are neighbouring points at the same step, so equal multiples of m put several zero factors into ONE shared inversion, and a call of
    `group` such points is a group made only of them; found neighbours with other k in the same group must not be harmed.  With more chunks per
    point the zero factors of neighbouring points meet in one group as well, `span` lanes apart."""
    group, chunk, _ = plan
    bb = 8
    m = 1 << bb
    eng.prepare_dlog(bb)
    assert chunk & (chunk - 1) == 0
    for bits in (bb + chunk.bit_length() - 1, bb + chunk.bit_length() + 2):
        top = 1 << (bits - bb)
        for j in (0, 3, chunk - 1, top - 1):
            only = np.full(group + 3, j * m)
            k, st = eng.dlog_base(DC.encode_multiples(only), bits)
            assert not st.any() and (k == only).all(), (bits, j)
            mixed = np.array([j * m, j * m + 1, j * m, 5, j * m, j * m, (j + 1) * m - 1, j * m] * 40)
            k, st = eng.dlog_base(DC.encode_multiples(mixed), bits)
            assert not st.any() and (k == mixed).all(), (bits, j)
    # the identity itself between points that do not decode and points that are never found
    junk = PC.enc_rows([PC.invalid_points()[0], PC.IDENTITY, DC.without_logarithm()[0], PC.IDENTITY, PC.IDENTITY, PC.invalid_points()[1]])
    k, st = eng.dlog_base(junk, 13)
    assert st.tolist() == [1, 0, 2, 0, 0, 1] and not k.any()


def test_one_point_with_many_chunks_and_several_slices(eng, plan):
    group, chunk, slice_chunks = plan
    bb, bits = 8, 24
    eng.prepare_dlog(bb)
    chunks = (1 << (bits - bb)) // chunk
    assert chunks > group                                              # one output, many work items, more than one workgroup
    s = slice_chunks(1) * chunk << bb
    ks = [0, 1, (1 << 24) - 1, (1 << 23) + 12345, 255, 256, chunk << bb, (chunk << bb) - 1]
    ks += [x for x in (s - 1, s, s + 1) if x < (1 << bits)]
    for k0 in ks:
        k, st = eng.dlog_base(DC.encode_multiples([k0]), bits)
        assert st[0] == DC.FOUND and int(k[0]) == k0, k0
    k, st = eng.dlog_base(DC.encode_multiples([1 << 24]), bits)
    assert st[0] == DC.NOT_FOUND and k[0] == 0
    # one output behind several launches whatever the slice length is: a range of three slices, the logarithm in the last one and at its edges
    wide = bb + int(np.ceil(np.log2(3 * slice_chunks(1) * chunk)))
    if wide <= 40:
        for k0 in ((1 << wide) - 1, s - 1, s, s + 1, 2 * s + 77):
            k, st = eng.dlog_base(DC.encode_multiples([k0]), wide)
            assert st[0] == DC.FOUND and int(k[0]) == k0, k0
    # many points: a launch covers only a few chunks of each, so a modest range is several launches too
    n = 300
    per = slice_chunks(n)
    bits2 = bb + int(np.ceil(np.log2(3 * per * chunk)))
    top = (1 << bits2) - 1
    kk = np.array([top - i * 977 for i in range(n)])
    k, st = eng.dlog_base(DC.encode_multiples(kk), bits2)
    assert not st.any() and (k == kk).all()


def test_4096_points_of_mixed_small_logarithms(eng):
    eng.prepare_dlog(12)
    pts, want = DC.small_mixed(4096, 20)
    k, st = eng.dlog_base(pts, 20)
    assert not st.any() and (k == want).all()
    eng.set_profiling(True)
    try:
        eng.dlog_base(pts[:100], 20)
        assert eng.last_kernels() == {"decode": ["k_dlog_prepare"], "terms": ["k_dlog_steps"]}
    finally:
        eng.set_profiling(False)


def test_preparing_another_size_replaces_the_table_and_changes_no_answer(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    pts, want_k, want_st = DC.operands(8, 17, chunk)
    e = Engine(0)
    try:
        assert e.dlog_baby_bits == 0
        check(e, pts, 17, want_k, want_st)                             # no table yet: the default size is built first
        default = e.dlog_baby_bits
        assert 4 <= default <= 22
        for bb in (5, 10, 5, default):
            e.prepare_dlog(bb)
            assert e.dlog_baby_bits == bb
            check(e, pts, 17, want_k, want_st)
        # the slots of the fixed-base registry are not touched
        reg = PC.enc_rows(list(PC.hashed_points()))
        e.prepare_fixed_points(reg)
        e.prepare_dlog(6)
        check(e, pts, 17, want_k, want_st)
    finally:
        e.close()


def test_results_do_not_depend_on_what_the_workspace_held(plan):
    from zkp_amd.engine import Engine
    group, chunk, _ = plan
    pts, want_k, want_st = DC.operands(8, 14, chunk)
    e = Engine(0, test_hooks=True)
    try:
        e.prepare_dlog(8)
        for word in (0xFFFFFFFF, 2, 0):
            e.debug_fill_workspace(8 << 20, word)
            check(e, pts, 14, want_k, want_st)
    finally:
        e.close()


def test_argument_errors_write_nothing(eng):
    lib, h = eng._lib, eng._h
    eng.prepare_dlog(8)
    pts = DC.encode_multiples([3, 4])
    out, st = np.full(2, 77, np.uint64), np.full(2, 9, np.uint8)
    P, O, ST = pts.ctypes.data, out.ctypes.data, st.ctypes.data
    assert lib.zkp_dlog_base(h, 0, None, 8, None, None) == 0 and lib.zkp_dlog_base_dev(h, 0, None, 8, None, None) == 0
    assert lib.zkp_dlog_base(None, 2, P, 8, O, ST) == ERR_ARG and lib.zkp_dlog_base_dev(None, 2, P, 8, O, ST) == ERR_ARG
    for args in ((None, 8, O, ST), (P, 8, None, ST), (P, 8, O, None), (P, 0, O, ST), (P, 49, O, ST), (P, 2**32 - 1, O, ST)):
        assert lib.zkp_dlog_base(h, 2, *args) == ERR_ARG, args
        assert lib.zkp_dlog_base_dev(h, 2, *args) == ERR_ARG, args     # (rejected before any pointer is used)
    assert lib.zkp_dlog_base(h, 2**31, P, 8, O, ST) == ERR_ARG
    assert (out == 77).all() and (st == 9).all()
    for bad in (0, 3, 23, 2**31):
        assert lib.zkp_ctx_prepare_dlog(h, bad) == ERR_ARG
    assert lib.zkp_ctx_prepare_dlog(None, 8) == ERR_ARG and lib.zkp_dlog_baby_bits(None) == 0
    assert eng.dlog_baby_bits == 8
    # a plan of more launches than the call accepts is refused before anything runs: 2^31 - 1 points of 2^44 giant steps
    eng.prepare_dlog(4)
    assert lib.zkp_dlog_base(h, 2**31 - 1, P, 48, O, ST) == ERR_ARG
    assert (out == 77).all() and (st == 9).all()
    assert T.lib().zkp_basepoint_dlog_batch(h, 2, P, 49, O, ST, 0) == -10
    with eng.capture():
        assert lib.zkp_ctx_prepare_dlog(h, 9) == ERR_ARG                # synchronous: not inside a capture
    assert eng.dlog_baby_bits == 4


def test_toolbox_routes_on_both_sides_of_the_threshold_and_agrees_with_the_host(eng, plan):
    group, chunk, _ = plan
    bb, bits = 8, 13
    eng.prepare_dlog(bb)
    pts, want_k, want_st = DC.operands(bb, bits, chunk)
    n = len(pts)
    host_bb, steps = T.get_dlog_baby_bits(), T.get_dlog_host_max_steps()
    T.set_dlog_baby_bits(bb)
    work = n * ((1 << (bits - bb)) + 128)                              # the call's host work in giant steps (128 for a point's decode and halving); the rule is per thread
    eng.set_profiling(True)
    try:
        host_k, host_st = T.basepoint_dlog(None, pts, bits)            # host and engine agree byte for byte
        k, st = check(eng, pts, bits, want_k, want_st)
        assert host_k.tobytes() == k.tobytes() and host_st.tobytes() == st.tobytes()
        T.set_dlog_host_max_steps(work - 1)
        k, st = T.basepoint_dlog(eng, pts, bits, threads=1)
        assert eng.last_kernels() == {"decode": ["k_dlog_prepare"], "terms": ["k_dlog_steps"]}     # the device ran it
        assert (k == want_k).all() and (st == want_st).all()
        eng.mul_base(PC.rows([5]))                                     # (leaves "k_mul_base" as the last call's kernel)
        T.set_dlog_host_max_steps(work)
        k, st = T.basepoint_dlog(eng, pts, bits, threads=1)
        assert eng.last_kernels() == {"terms": ["k_mul_base"]}         # the host threads, no kernel
        assert (k == want_k).all() and (st == want_st).all()
        k, st = T.basepoint_dlog(eng, np.concatenate([pts, pts[:1]]), bits, threads=1)       # one point more: the device again
        assert eng.last_kernels() == {"decode": ["k_dlog_prepare"], "terms": ["k_dlog_steps"]}
        assert (k[:-1] == want_k).all() and k[-1] == want_k[0]
    finally:
        eng.set_profiling(False)
        T.set_dlog_baby_bits(host_bb)
        T.set_dlog_host_max_steps(steps)


def test_the_default_threshold_routes_as_the_measurements_say(eng):
    """the shipped defaults (host table of 2^12 rows, 2,048 giant steps of host work per thread, threads counted up to 16): the shapes the
    measurements give to the host stay there, the next larger ones go to the device, and one thread keeps far less than sixteen"""
    assert T.get_dlog_baby_bits() == 12 and T.get_dlog_host_max_steps() == 2048
    eng.prepare_dlog(12)
    rng = np.random.default_rng(11)
    dev = {"decode": ["k_dlog_prepare"], "terms": ["k_dlog_steps"]}
    marker = {"terms": ["k_mul_base"]}
    eng.set_profiling(True)
    try:
        for n, bits, threads, on_host in ((1, 16, 16, True), (16, 16, 16, True), (227, 16, 16, True), (1, 24, 16, True), (1, 26, 16, True),
                                          (228, 16, 16, False), (256, 16, 16, False), (1, 27, 16, False), (1, 16, 1, True), (14, 16, 1, True),
                                          (1, 22, 1, True), (15, 16, 1, False), (1, 23, 1, False), (1, 24, 1, False), (16, 16, 0, True)):
            ks = rng.integers(0, 1 << bits, size=n)
            pts = DC.encode_multiples(ks)
            eng.mul_base(PC.rows([5]))                                 # (leaves "k_mul_base" as the last call's kernel)
            k, st = T.basepoint_dlog(eng, pts, bits, threads=threads)
            assert eng.last_kernels() == (marker if on_host else dev), (n, bits, threads)
            assert not st.any() and (k == ks.astype(np.uint64)).all(), (n, bits, threads)
    finally:
        eng.set_profiling(False)


def test_dev_form_on_a_side_stream_and_recorded_into_a_graph(plan):
    """zkp_dlog_base_dev on torch device buffers and a side stream; then recorded into a graph (after one plain call, which builds the table and
    the workspace) whose two replays follow new inputs placed in the same buffers.  The range needs several slices: the launches follow each
    other inside the recording."""
    torch = _torch()
    from zkp_amd.engine import Engine
    group, chunk, slice_chunks = plan
    bb = 6
    pts, want_k, want_st, bits = slice_cases(bb, plan)
    n = len(pts)
    rng = np.random.default_rng(5)
    perms = [np.arange(n), rng.permutation(n), rng.permutation(n)]
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    with e.capture():                                                  # no table yet: the call cannot be recorded
        assert e._lib.zkp_dlog_base_dev(e._h, n, 256, bits, 256, 256) == ERR_ARG
    e.prepare_dlog(bb)
    d_pts = torch.from_numpy(pts).to("cuda:0")
    d_out = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def enqueue():
        e.dlog_base_dev(n, d_pts.data_ptr(), bits, d_out.data_ptr(), d_st.data_ptr())

    def check_dev(p):
        assert (d_out.cpu().numpy().view(np.uint64) == want_k[p]).all() and (d_st.cpu().numpy() == want_st[p]).all()

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
    cap.graph.close()
    e.close()


def test_the_elgamal_amounts_example_on_the_engine(eng):
    spec = importlib.util.spec_from_file_location("elgamal_amounts_batch", os.path.join(ROOT, "examples", "elgamal_amounts_batch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, bits = 256, 24
    eng.prepare_dlog(12)
    amounts = np.random.default_rng(9).integers(0, 1 << bits, size=n)
    amounts[:4] = [0, 1, (1 << bits) - 1, 1 << bits]                   # the last of them is out of range
    r = mod.run(eng, n, bits, key=bytes(range(1, 33)), amounts=amounts)
    assert r["accepted"] == n and r["rejected"] == n and r["match"]
    assert r["status"][3] == 2 and (np.delete(r["status"], 3) == 0).all()
    assert (np.delete(r["recovered"], 3) == np.delete(amounts, 3).astype(np.uint64)).all()
    assert (r["aB"] == DC.encode_multiples(amounts)).all()
    host = mod.run(None, 16, 12, key=bytes(range(1, 33)), amounts=amounts[:16] % 4096)      # the same secrets on the host backend
    again = mod.run(eng, 16, 12, key=bytes(range(1, 33)), amounts=amounts[:16] % 4096)
    for k in ("C1", "C2", "Z", "aB", "recovered", "status"):
        assert (host[k] == again[k]).all(), k

"""Batched scalars mod l on the MI355X: k_sc_invert, k_sc_from_wide, k_sc_muladd and k_sc_hash_sha512 behind zkp_sc_* / zkp_sc_*_dev,
zkp_sc_random (the device ChaCha20 stream through k_sc_from_wide) and the toolbox's zkp_scalar_*_batch, whose device route the GPU tests
take at every size.  Expected values are Python integers, hashlib and zkp_chacha20_block; the host backend (the same sc25519.h and
sha512.h compiled by g++) must agree byte for byte.  Operands: the 256-bit edge catalogue of tests/scalar_edge_cases.py."""
import hashlib
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.scalar_edge_cases import L, VALUES, random_256
from tests.test_host_hash_from_bytes import csr_messages, random_batch, sweep_batch
from tests.test_host_scalar_ops import EDGES, WIDE_EDGES, chacha_block, ints, rows, want_hash
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]
GRID_CAP_BLOCKS = 2048                                        # kMaxBlocks of zkp_kernels.hip: the launchers' grid cap
N_STRIDE = GRID_CAP_BLOCKS * 256 + 257                        # the grid-stride loop runs a second, partial round
KEY, NONCE = bytes(range(32)), 0x1122334455667788
CAT = VALUES + [v for v in EDGES if v not in VALUES]


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def inv(v):
    return pow(v % L, L - 2, L)


def sample_indices(n, seed):
    """4,096 indices of range(n) that contain the first 512 and the last 512 (the second round of the grid-stride loop lives at the end)"""
    rng = random.Random(seed)
    return sorted(set(range(512)) | set(range(n - 512, n)) | set(rng.sample(range(512, n - 512), 4096 - 1024)))


@pytest.mark.parametrize("n", SIZES)
def test_every_call_at_wavefront_and_block_edges(eng, n):
    vals = random_256(100 + n, 3 * n)
    a, b, c = vals[:n], vals[n:2 * n], vals[2 * n:]
    A, B, Cc = (rows(x) if n else np.zeros((0, 32), np.uint8) for x in (a, b, c))
    W = np.concatenate([A, B], axis=1)
    for route in (eng.scalar_invert, lambda x: T.scalar_invert(eng, x)):
        assert ints(route(A)) == [inv(v) for v in a]
    for route in (eng.scalar_from_wide, lambda x: T.scalar_from_wide(eng, x)):
        assert ints(route(W)) == [(x + (y << 256)) % L for x, y in zip(a, b)]
    if n:
        for route in (eng.scalar_muladd, lambda *x: T.scalar_muladd(eng, *x)):
            assert ints(route(A, B, Cc)) == [(x * y + z) % L for x, y, z in zip(a, b, c)]
            assert ints(route(A, B)) == [x * y % L for x, y in zip(a, b)]
    else:
        assert eng._lib.zkp_sc_muladd(eng._h, 0, None, 1, None, 1, None, 1, None) == 0
        assert T.lib().zkp_scalar_muladd_batch(eng._h, 0, None, 1, None, 1, None, 1, 0, None) == 0
    data, offsets = random_batch(n, 900 + n)
    msgs = csr_messages(data, offsets)
    for route in (eng.scalar_hash_from_bytes_sha512_csr, lambda d, o: T.scalar_hash_from_bytes_sha512_csr(eng, d, o)):
        assert ints(route(data, offsets)) == want_hash(msgs)
    want_rand = [int.from_bytes(chacha_block(KEY, i, NONCE), "little") % L for i in range(n)]
    assert ints(eng.scalar_random(n, KEY, NONCE)) == want_rand
    assert ints(T.scalar_random(eng, n, KEY, NONCE)) == want_rand


@pytest.mark.parametrize("op", ["invert", "from_wide", "muladd", "hash", "random"])
def test_grid_stride_second_round(eng, op):
    n = N_STRIDE
    rng = np.random.default_rng(n)
    pick = sample_indices(n, 5)
    assert pick[:512] == list(range(512)) and pick[-512:] == list(range(n - 512, n)) and len(pick) == 4096
    if op == "invert":
        A = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        got = eng.scalar_invert(A)
        assert ints(got[pick]) == [inv(v) for v in ints(A[pick])]                      # (524,545 modular powers take longer than a few seconds)
        assert (got == T.scalar_invert(None, A, threads=16)).all()
    elif op == "from_wide":
        W = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        got = eng.scalar_from_wide(W)
        assert ints(got) == [v % L for v in ints(W)]
    elif op == "muladd":
        A, B, Cc = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(3))
        got = eng.scalar_muladd(A, B, Cc)
        assert ints(got) == [(x * y + z) % L for x, y, z in zip(ints(A), ints(B), ints(Cc))]
    elif op == "hash":
        data, offsets = random_batch(n, 11, max_len=40)
        got = eng.scalar_hash_from_bytes_sha512_csr(data, offsets)
        assert ints(got) == want_hash(csr_messages(data, offsets))
    else:
        got = eng.scalar_random(n, KEY, NONCE)
        assert ints(got[pick]) == [int.from_bytes(chacha_block(KEY, i, NONCE), "little") % L for i in pick]
        assert (got == T.scalar_random(None, n, KEY, NONCE, threads=16)).all()


def test_edge_operands_at_index_0_the_last_index_and_both_sides_of_lane_boundaries(eng):
    """round j puts catalogue value j + t at the t-th of the positions 0, 63, 64, 65, 255, 256, 257 and n - 1 (its neighbours in the
    other operands): after len(CAT) rounds every value has stood at every position.  The rest is random and the same in every round."""
    n, m = 300, len(CAT)
    pos = [0, 63, 64, 65, 255, 256, 257, n - 1]
    fill = random_256(300, 3 * n)
    base = [fill[:n], fill[n:2 * n], fill[2 * n:]]
    want_inv = [inv(v) for v in base[0]]
    want_wide = [(x + (y << 256)) % L for x, y in zip(base[0], base[1])]
    want_mul = [(x * y + z) % L for x, y, z in zip(*base)]
    arrs = [rows(x) for x in base]
    for j in range(m):
        wi, ww, wm = list(want_inv), list(want_wide), list(want_mul)
        for t, p in enumerate(pos):
            x, y, z = CAT[(j + t) % m], CAT[(j + t + 1) % m], CAT[(j + t + 2) % m]
            for arr, v in zip(arrs, (x, y, z)):
                arr[p] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
            wi[p], ww[p], wm[p] = inv(x), (x + (y << 256)) % L, (x * y + z) % L
        A, B, Cc = arrs
        got = eng.scalar_invert(A)
        assert ints(got) == wi, j
        assert (got == T.scalar_invert(None, A)).all()
        W = np.concatenate([A, B], axis=1)
        got = eng.scalar_from_wide(W)
        assert ints(got) == ww, j
        assert (got == T.scalar_from_wide(None, W)).all()
        got = eng.scalar_muladd(A, B, Cc)
        assert ints(got) == wm, j
        assert (got == T.scalar_muladd(None, A, B, Cc)).all()
    wide = WIDE_EDGES + [0] * (n - len(WIDE_EDGES) - 1) + [WIDE_EDGES[3]]
    assert ints(eng.scalar_from_wide(rows(wide, 64))) == [v % L for v in wide]


def test_dev_forms_on_torch_buffers(eng):
    """the _dev forms on torch-allocated device buffers, queued on a torch stream: in-place inversion, every stride combination of muladd
    at n = 257 with out aliasing a stride-1 operand, from_wide, random, and the hash with messages at an odd device address"""
    torch = _torch()
    from zkp_amd.engine import Engine
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    dev = lambda x: torch.from_numpy(x).to("cuda:0")                          # noqa: E731
    n = 257
    vals = CAT + random_256(41, n - len(CAT))
    assert len(vals) == n
    a, b, c = vals, vals[::-1], vals[7:] + vals[:7]
    d_a, d_b, d_c = dev(rows(a)), dev(rows(b)), dev(rows(c))
    d_out = torch.zeros((n + 2, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    # inversion into rows 1 .. n of a larger buffer, then in place
    e.scalar_invert_dev(n, d_a.data_ptr(), d_out.data_ptr() + 32)
    e.synchronize()
    out = d_out.cpu().numpy()
    assert ints(out[1:n + 1]) == [inv(v) for v in a] and not out[0].any() and not out[n + 1].any()
    d_io = d_a.clone()
    torch.cuda.synchronize()
    e.scalar_invert_dev(n, d_io.data_ptr(), d_io.data_ptr())
    e.synchronize()
    assert (d_io.cpu().numpy() == out[1:n + 1]).all()
    # from_wide
    d_w = dev(np.concatenate([rows(a), rows(b)], axis=1))
    torch.cuda.synchronize()
    e.scalar_from_wide_dev(n, d_w.data_ptr(), d_out.data_ptr() + 32)
    e.synchronize()
    assert ints(d_out.cpu().numpy()[1:n + 1]) == [(x + (y << 256)) % L for x, y in zip(a, b)]
    # muladd: all eight stride combinations and c = NULL; out = the first stride-1 operand when there is one
    for sa, sb, sc in list(itertools.product((0, 1), repeat=3)) + [(1, 1, None)]:
        ops = [d_a.clone(), d_b.clone(), d_c.clone()]
        alias = [k for k, s in enumerate((sa, sb, sc)) if s == 1]
        d_o = ops[alias[0]] if alias else torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        e.scalar_muladd_dev(n, ops[0].data_ptr(), sa, ops[1].data_ptr(), sb, None if sc is None else ops[2].data_ptr(), sc or 0, d_o.data_ptr())
        e.synchronize()
        want = [(a[i * sa] * b[i * sb] + (0 if sc is None else c[i * sc])) % L for i in range(n)]
        assert ints(d_o.cpu().numpy()) == want, (sa, sb, sc)
    # random
    e.scalar_random_dev(n, KEY, NONCE, d_out.data_ptr() + 32)
    e.synchronize()
    assert (d_out.cpu().numpy()[1:n + 1] == T.scalar_random(None, n, KEY, NONCE)).all()
    # hash: messages at an odd device address
    data, offsets = random_batch(n, 77)
    lead = 3
    d_data = torch.zeros(lead + len(data), dtype=torch.uint8, device="cuda:0")
    d_data[lead:] = dev(data)
    d_off = dev(offsets.view(np.int64))
    torch.cuda.synchronize()
    e.scalar_hash_from_bytes_sha512_dev(n, d_data.data_ptr() + lead, len(data), d_off.data_ptr(), d_out.data_ptr() + 32)
    e.synchronize()
    out = d_out.cpu().numpy()
    assert ints(out[1:n + 1]) == want_hash(csr_messages(data, offsets)) and not out[0].any() and not out[n + 1].any()
    e.close()


def test_hash_sweep_and_rebased_sub_batch(eng):
    data, offsets, marks = sweep_batch()
    assert {0, 111, 112, 127, 128, 239, 240, 1000, 65536} <= {n for _, n, _ in marks}
    got = eng.scalar_hash_from_bytes_sha512_csr(data, offsets)
    assert ints(got) == want_hash(csr_messages(data, offsets))
    assert (got == T.scalar_hash_from_bytes_sha512_csr(None, data, offsets, threads=16)).all()
    # a batch that does not start at offset 0 of the buffer: the upload is rebased, the start offsets mod 4 change
    assert (eng.scalar_hash_from_bytes_sha512_csr(data, offsets[5:400]) == got[5:399]).all()
    assert (T.scalar_hash_from_bytes_sha512_csr(eng, data, offsets[5:400]) == got[5:399]).all()


def test_timing_kinds(eng):
    n = 4096
    rng = np.random.default_rng(1)
    A, B = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for _ in range(2))
    data, offsets = random_batch(n, 3)
    calls = {"invert": lambda: eng.scalar_invert(A), "from_wide": lambda: eng.scalar_from_wide(np.concatenate([A, B], axis=1)),
             "muladd": lambda: eng.scalar_muladd(A, B, A), "random": lambda: eng.scalar_random(n, KEY, NONCE),
             "hash": lambda: eng.scalar_hash_from_bytes_sha512_csr(data, offsets)}
    eng.set_profiling(True)
    try:
        for name, call in calls.items():
            call()
            timing, _ = eng.last_timing()
            print(name, timing)
            if name == "hash":                                                 # one kernel, filed under its SHA-512 stage
                assert timing["transcript"] > 0, name
            else:
                assert timing["scalars"] > 0, name
    finally:
        eng.set_profiling(False)


def test_argument_errors(eng):
    lib = eng._lib
    buf = np.zeros((4, 64), np.uint8)
    out = np.zeros((4, 32), np.uint8)
    ok = np.array([0, 1, 2, 3, 4], np.uint64)
    dec = np.array([0, 3, 2, 3, 4], np.uint64)
    key = np.zeros(32, np.uint8)
    p = lambda x: x.ctypes.data                                                # noqa: E731
    ARG = -2                                                                   # ZKP_ERR_ARG
    assert lib.zkp_sc_invert(eng._h, 4, None, p(out)) == ARG and lib.zkp_sc_invert(eng._h, 4, p(buf), None) == ARG
    assert lib.zkp_sc_invert(eng._h, 1 << 31, p(buf), p(out)) == ARG and lib.zkp_sc_invert(None, 4, p(buf), p(out)) == ARG
    assert lib.zkp_sc_from_wide(eng._h, 4, None, p(out)) == ARG and lib.zkp_sc_from_wide(eng._h, 4, p(buf), None) == ARG
    assert lib.zkp_sc_from_wide(eng._h, 1 << 31, p(buf), p(out)) == ARG
    assert lib.zkp_sc_muladd(eng._h, 4, None, 1, p(buf), 1, None, 1, p(out)) == ARG
    assert lib.zkp_sc_muladd(eng._h, 4, p(buf), 1, p(buf), 1, None, 1, None) == ARG
    for bad in ((2, 1, 1), (1, 2, 1), (1, 1, 2)):
        assert lib.zkp_sc_muladd(eng._h, 4, p(buf), bad[0], p(buf), bad[1], p(buf), bad[2], p(out)) == ARG
        assert lib.zkp_sc_muladd_dev(eng._h, 4, 256, bad[0], 256, bad[1], 256, bad[2], 256) == ARG
        assert T.lib().zkp_scalar_muladd_batch(eng._h, 4, p(buf), bad[0], p(buf), bad[1], p(buf), bad[2], 0, p(out)) == -10
    assert lib.zkp_sc_muladd(eng._h, 1 << 31, p(buf), 1, p(buf), 1, None, 1, p(out)) == ARG
    assert lib.zkp_sc_hash_from_bytes_sha512(eng._h, 4, p(buf), p(dec), p(out)) == ARG
    assert lib.zkp_sc_hash_from_bytes_sha512(eng._h, 4, None, p(ok), p(out)) == ARG
    assert lib.zkp_sc_hash_from_bytes_sha512(eng._h, 1 << 31, p(buf), p(ok), p(out)) == ARG
    assert lib.zkp_sc_random(eng._h, 4, None, 0, p(out)) == ARG and lib.zkp_sc_random(eng._h, 4, p(key), 0, None) == ARG
    # _dev forms: NULL, size and alignment are checked before anything is queued
    assert lib.zkp_sc_invert_dev(eng._h, 4, None, 256) == ARG and lib.zkp_sc_invert_dev(eng._h, 4, 256, 264) == ARG
    assert lib.zkp_sc_invert_dev(eng._h, 1 << 31, 256, 256) == ARG
    assert lib.zkp_sc_from_wide_dev(eng._h, 4, 264, 256) == ARG and lib.zkp_sc_from_wide_dev(eng._h, 4, 256, None) == ARG
    assert lib.zkp_sc_muladd_dev(eng._h, 4, 256, 1, 264, 1, None, 1, 256) == ARG and lib.zkp_sc_muladd_dev(eng._h, 4, 256, 1, 256, 1, 264, 1, 256) == ARG
    assert lib.zkp_sc_random_dev(eng._h, 4, p(key), 0, 264) == ARG and lib.zkp_sc_random_dev(eng._h, 4, None, 0, 256) == ARG
    assert lib.zkp_sc_hash_from_bytes_sha512_dev(eng._h, 3, None, 0, 12, 16) == ARG           # d_offsets not 8-byte aligned
    assert lib.zkp_sc_hash_from_bytes_sha512_dev(eng._h, 3, None, 0, 8, 24) == ARG            # d_out not 16-byte aligned
    assert lib.zkp_sc_hash_from_bytes_sha512_dev(eng._h, 3, None, 64, 8, 16) == ARG
    for f, args in ((lib.zkp_sc_invert, (None, None)), (lib.zkp_sc_invert_dev, (None, None)), (lib.zkp_sc_from_wide, (None, None)),
                    (lib.zkp_sc_from_wide_dev, (None, None)), (lib.zkp_sc_muladd, (None, 1, None, 1, None, 1, None)),
                    (lib.zkp_sc_muladd_dev, (None, 1, None, 1, None, 1, None)), (lib.zkp_sc_random, (None, 0, None)),
                    (lib.zkp_sc_random_dev, (None, 0, None)), (lib.zkp_sc_hash_from_bytes_sha512, (None, None, None)),
                    (lib.zkp_sc_hash_from_bytes_sha512_dev, (None, 0, None, None))):
        assert f(eng._h, 0, *args) == 0                                        # n = 0 is a no-op
    assert not out.any()
    assert T.lib().zkp_scalar_hash_from_bytes_sha512_batch(eng._h, 4, p(buf), p(dec), 0, p(out)) == -10
    assert T.lib().zkp_scalar_invert_batch(eng._h, 4, None, 0, p(out)) == -10


def test_voprf_example_runs_as_a_child_process():
    """examples/voprf_batch.py 256: a blinded evaluation on product calls alone -- proofs verify, r^-1 unblinds to k T, a replaced Z fails.
    (Its multiplications are Engine.msm_many, which has no host-backend form: the flow cannot run with eng=None, so there is no CPU twin.)"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "voprf_batch.py"), "256"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify" in r.stdout and "rejected" in r.stdout

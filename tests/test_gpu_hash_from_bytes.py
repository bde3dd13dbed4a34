"""RistrettoPoint::hash_from_bytes::<Sha512> on the MI355X: k_sha512_csr (SHA-512 over a CSR batch of messages) then k_from_uniform, behind
zkp_hash_from_bytes_sha512 / _dev and the toolbox's zkp_hash_from_bytes_sha512_batch; the raw digests through the test hook
zkp_debug_sha512; and the reference's create_batch_and_batch_verify (tests/zkp.rs:115-175) for 4,096 messages on product calls.
Checked against hashlib, the host backend (the same sha512.h and ge25519.h on the host) and the oracle.  Only valid offsets go to the
GPU: the kernel's clamp is sha512.h's sha512_clamp, which tests/test_host_hash_from_bytes.py checks under sanitizers."""
import hashlib

import numpy as np
import pytest

from oracle import cbind as C
from tests.test_host_hash_from_bytes import BASEPOINT, HEX_H, csr_messages, random_batch, sweep_batch, want_points
from tests.test_host_hash_to_group import RFC_A3
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    C.build()
    e = Engine(0)
    yield e
    e.close()


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def test_debug_digests_equal_hashlib_over_the_length_and_offset_sweep():
    from zkp_amd.engine import Engine
    data, offsets, marks = sweep_batch()
    msgs = csr_messages(data, offsets)
    e = Engine(0, test_hooks=True)
    try:
        got = e.debug_sha512(data, offsets)
        assert [bytes(d) for d in got] == [hashlib.sha512(m).digest() for m in msgs]
        lens = {n for _, n, _ in marks}
        assert {111, 112, 127, 128, 239, 240, 1000, 65536} <= lens
        # a batch that does not start at offset 0 of the buffer: the upload is rebased, the start offsets mod 4 change
        got2 = e.debug_sha512(data, offsets[5:400])
        assert (got2 == got[5:399]).all()
        assert e.debug_sha512(data, offsets[:1]).shape == (0, 64)
    finally:
        e.close()


def test_sweep_rfc_vectors_and_c_example_generator_on_the_device(eng):
    data, offsets, _ = sweep_batch()
    got = eng.hash_from_bytes_sha512_csr(data, offsets)
    assert (got == T.hash_from_bytes_sha512_csr(None, data, offsets, threads=16)).all()
    assert (got == want_points(csr_messages(data, offsets))).all()
    assert [bytes(g) for g in eng.hash_from_bytes_sha512([m for m, _ in RFC_A3])] == [bytes.fromhex(h) for _, h in RFC_A3]
    assert bytes(eng.hash_from_bytes_sha512([BASEPOINT])[0]).hex() == HEX_H
    assert eng.hash_from_bytes_sha512([]).shape == (0, 32)


@pytest.mark.parametrize("n", [1, 257, 4096, 1 << 20])
def test_random_batches_device_host_and_oracle_agree(eng, n):
    data, offsets = random_batch(n, n)
    eng.set_profiling(True)
    try:
        got = T.hash_from_bytes_sha512_csr(eng, data, offsets)             # the gpu tests set host_max_terms to 0: the device route
        timing, _ = eng.last_timing()
    finally:
        eng.set_profiling(False)
    assert timing["transcript"] > 0 and timing["decode"] > 0
    assert (got == eng.hash_from_bytes_sha512_csr(data, offsets)).all()
    assert (got == T.hash_from_bytes_sha512_csr(None, data, offsets, threads=16)).all()
    rng = np.random.default_rng(n + 1)
    pick = np.sort(rng.choice(n, size=min(n, 2048), replace=False))
    msgs = [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in pick]
    assert (got[pick] == want_points(msgs)).all()


def test_argument_errors(eng):
    lib = eng._lib
    data = np.arange(64, dtype=np.uint8)
    out = np.zeros((3, 32), np.uint8)
    dec = np.array([0, 10, 5, 20], np.uint64)
    ok = np.array([0, 5, 10, 20], np.uint64)
    p = lambda a: a.ctypes.data                                                # noqa: E731
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 3, p(data), p(dec), p(out)) == -2          # ZKP_ERR_ARG
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 3, None, p(ok), p(out)) == -2
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 3, p(data), None, p(out)) == -2
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 3, p(data), p(ok), None) == -2
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 1 << 31, p(data), p(ok), p(out)) == -2
    assert lib.zkp_hash_from_bytes_sha512(None, 3, p(data), p(ok), p(out)) == -2
    assert lib.zkp_hash_from_bytes_sha512(eng._h, 0, None, None, None) == 0
    assert lib.zkp_hash_from_bytes_sha512_dev(eng._h, 0, None, 0, None, None) == 0
    assert lib.zkp_hash_from_bytes_sha512_dev(eng._h, 3, None, 64, None, None) == -2
    assert lib.zkp_hash_from_bytes_sha512_dev(eng._h, 1 << 31, None, 0, 8, 16) == -2
    assert lib.zkp_hash_from_bytes_sha512_dev(eng._h, 3, None, 0, 12, 16) == -2                # d_offsets not 8-byte aligned
    assert lib.zkp_hash_from_bytes_sha512_dev(eng._h, 3, None, 0, 8, 24) == -2                 # d_out not 16-byte aligned
    assert not out.any()
    # the toolbox checks the offsets before it picks a backend
    assert T.lib().zkp_hash_from_bytes_sha512_batch(eng._h, 3, p(data), p(dec), 0, p(out)) == -10
    assert not out.any()


def test_dev_entry_plain_and_captured_into_a_table_row(eng):
    """zkp_hash_from_bytes_sha512_dev on torch device buffers: messages at an odd device address, output into rows 5.. of a larger
    [rows][32] table (the d_table layout of the fused flows), queued on the context's stream, and recorded into a graph whose replay
    follows new message bytes placed in the same buffer"""
    torch = _torch()
    from zkp_amd.engine import Engine
    n, lead, row0, rows = 3000, 3, 5, 3100
    data_a, offsets = random_batch(n, 77)
    rng = np.random.default_rng(78)
    data_b = rng.integers(0, 256, size=len(data_a), dtype=np.uint8)
    want_a = T.hash_from_bytes_sha512_csr(None, data_a, offsets)
    want_b = T.hash_from_bytes_sha512_csr(None, data_b, offsets)
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_data = torch.zeros(lead + len(data_a), dtype=torch.uint8, device="cuda:0")
    d_data[lead:] = torch.from_numpy(data_a).to("cuda:0")
    d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda:0")
    d_table = torch.zeros((rows, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (n, d_data.data_ptr() + lead, len(data_a), d_off.data_ptr(), d_table.data_ptr() + 32 * row0)
    e.hash_from_bytes_sha512_dev(*args)
    e.synchronize()
    table = d_table.cpu().numpy()
    assert (table[row0:row0 + n] == want_a).all()
    assert not table[:row0].any() and not table[row0 + n:].any()
    d_table.zero_()
    torch.cuda.synchronize()
    with e.capture() as cap:
        e.hash_from_bytes_sha512_dev(*args)
    assert not bool(d_table.any().item())                               # recorded, not run
    cap.graph.launch()
    e.synchronize()
    assert (d_table.cpu().numpy()[row0:row0 + n] == want_a).all()
    d_data[lead:] = torch.from_numpy(data_b).to("cuda:0")
    torch.cuda.synchronize()
    cap.graph.launch()
    e.synchronize()
    table = d_table.cpu().numpy()
    assert (table[row0:row0 + n] == want_b).all()
    assert not table[:row0].any() and not table[row0 + n:].any()
    cap.graph.close()
    e.close()


def test_create_batch_and_batch_verify_for_4096_messages(eng):
    """tests/zkp.rs:115-175 for 4,096 messages on product calls (examples/dleq_messages_batch.py): the batch verifies, and fails when one
    message is changed on the verifier's side.  The first four generators equal the oracle's hash of the reference's four messages."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "dleq_messages_batch.py")
    spec = importlib.util.spec_from_file_location("dleq_messages_batch", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    msgs = ex.messages_for(4096)
    assert msgs[:4] == [b"One message", b"Another message", b"A third message", b"A fourth message"] and len(set(msgs)) == 4096
    assert (eng.hash_from_bytes_sha512(msgs[:4]) == want_points(msgs[:4])).all()
    ok, ok_changed = ex.run(eng, msgs)
    assert ok and not ok_changed

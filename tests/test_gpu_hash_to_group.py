"""Hash to the group on the MI355X: k_from_uniform behind zkp_from_uniform_bytes / _dev, the device-transcript route of
zkp_hash_to_group_batch (zkp_fused_hash_to_group), and a batch of the reference's VRF (tests/sig_and_vrf_example.rs) built from product
calls alone.  Checked against the host backend (the same formulas over the 5 x 51 host field), the oracle and RFC 9496's vectors."""
import hashlib

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests.test_host_hash_to_group import RFC_A3, edge_inputs, model_blob, oracle_map
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

pytestmark = pytest.mark.gpu
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


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


def test_rfc_vectors_and_edge_inputs_on_the_device(eng):
    wide = np.frombuffer(b"".join(hashlib.sha512(m).digest() for m, _ in RFC_A3), np.uint8).reshape(-1, 64)
    want = [bytes.fromhex(h) for _, h in RFC_A3]
    assert [bytes(g) for g in eng.from_uniform_bytes(wide)] == want
    assert [bytes(g) for g in T.hash_from_bytes_sha512(eng, [m for m, _ in RFC_A3])] == want
    rows = edge_inputs()
    got = eng.from_uniform_bytes(rows)
    assert (got == oracle_map(rows)).all()
    assert (got == T.from_uniform_bytes(None, rows)).all()
    assert eng.from_uniform_bytes(np.zeros((0, 64), np.uint8)).shape == (0, 32)


@pytest.mark.parametrize("n", [1, 255, 257, 4096, 1 << 20])
def test_random_batches_equal_host_backend_and_oracle(eng, n):
    rng = np.random.default_rng(n)
    rows = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    got = eng.from_uniform_bytes(rows)
    assert (got == T.from_uniform_bytes(None, rows)).all()
    pick = rng.choice(n, size=min(n, 4096), replace=False)
    assert (got[pick] == oracle_map(rows[pick])).all()
    # the toolbox call routes this size to the device (the gpu tests set host_max_terms to 0) and gives the same bytes
    if n <= 4096:
        assert (T.from_uniform_bytes(eng, rows) == got).all()


def test_argument_errors(eng):
    lib = eng._lib
    out = np.zeros((2, 32), np.uint8)
    inp = np.zeros((2, 64), np.uint8)
    assert lib.zkp_from_uniform_bytes(eng._h, 2, None, out.ctypes.data) == -2                  # ZKP_ERR_ARG
    assert lib.zkp_from_uniform_bytes(eng._h, 2, inp.ctypes.data, None) == -2
    assert lib.zkp_from_uniform_bytes_dev(eng._h, 2, None, None) == -2
    assert lib.zkp_from_uniform_bytes(eng._h, 0, None, None) == 0
    assert lib.zkp_from_uniform_bytes_dev(eng._h, 0, None, None) == 0
    assert lib.zkp_from_uniform_bytes(None, 2, inp.ctypes.data, out.ctypes.data) == -2
    ts = np.stack([T.Transcript(b"a").state, T.Transcript(b"bb").state])     # different STROBE positions
    assert lib.zkp_fused_hash_to_group(eng._h, 2, ts.ctypes.data, b"output", out.ctypes.data) == -2
    assert lib.zkp_fused_hash_to_group(eng._h, 2, ts.ctypes.data, None, out.ctypes.data) == -2
    assert not out.any()


def test_dev_entry_plain_and_captured(eng):
    """zkp_from_uniform_bytes_dev on torch device buffers: queued on the context's stream, and recorded into a graph (one kernel: a linear
    graph) whose replay follows new inputs placed in the same buffer"""
    torch = _torch()
    from zkp_amd.engine import Engine
    rng = np.random.default_rng(11)
    n = 3000
    a, b = (rng.integers(0, 256, size=(n, 64), dtype=np.uint8) for _ in range(2))
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_in = torch.from_numpy(a).to("cuda:0")
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    e.from_uniform_bytes_dev(n, d_in.data_ptr(), d_out.data_ptr())
    e.synchronize()
    want_a = T.from_uniform_bytes(None, a)
    assert (d_out.cpu().numpy() == want_a).all()
    d_out.zero_()
    torch.cuda.synchronize()
    with e.capture() as cap:
        e.from_uniform_bytes_dev(n, d_in.data_ptr(), d_out.data_ptr())
    assert not bool(d_out.any().item())                                 # recorded, not run
    cap.graph.launch()
    e.synchronize()
    assert (d_out.cpu().numpy() == want_a).all()
    d_in.copy_(torch.from_numpy(b).to("cuda:0"))
    torch.cuda.synchronize()
    cap.graph.launch()
    e.synchronize()
    assert (d_out.cpu().numpy() == T.from_uniform_bytes(None, b)).all()
    cap.graph.close()
    e.close()


def _function_transcripts(msgs, dom=b"My VRF Application"):
    ts = []
    for m in msgs:
        t = T.Transcript(dom)
        t.append_message(b"msg", m)
        ts.append(t)
    return np.stack([t.state for t in ts])


def _model_hash(msgs, dom=b"My VRF Application"):
    hs, blobs = [], []
    for m in msgs:
        t = M.Transcript(dom)
        t.append_message(b"msg", m)
        hs.append(C.from_uniform_bytes(t.challenge_bytes(b"output", 64)))
        blobs.append(model_blob(t))
    return hs, blobs


def test_hash_to_group_device_and_host_transcript_routes_agree(eng):
    rng = np.random.default_rng(12)
    n = 600
    assert n >= T.get_fused_min_batch()
    aligned = [rng.bytes(24) for _ in range(n)]
    ragged = [rng.bytes(int(rng.integers(0, 200))) for _ in range(n)]
    for msgs in (aligned, ragged):
        want_h, want_blobs = _model_hash(msgs)
        ts = _function_transcripts(msgs)
        eng.set_profiling(True)
        try:
            got = T.hash_to_group(eng, ts)
            timing, _ = eng.last_timing()
            kernels = eng.last_kernels()
        finally:
            eng.set_profiling(False)
        assert [bytes(g) for g in got] == want_h
        assert [r.tobytes() for r in ts] == want_blobs
        if msgs is aligned:                                             # the device-transcript route ran the transcript kernel
            assert timing["transcript"] > 0 and timing["decode"] > 0 and "transcript" in kernels
        # a second challenge agrees with the model: the states were advanced, not just copied
        t0 = T.Transcript(_state=ts[n // 2])
        m0 = M.Transcript(b"My VRF Application")
        m0.append_message(b"msg", msgs[n // 2])
        m0.challenge_bytes(b"output", 64)
        assert t0.challenge_bytes(b"next", 32) == m0.challenge_bytes(b"next", 32)
    # the same aligned batch on both routes: identical outputs and states
    ts_dev, ts_host = _function_transcripts(aligned), _function_transcripts(aligned)
    out_dev = T.hash_to_group(eng, ts_dev)
    old = T.get_fused_min_batch()
    try:
        T.set_fused_min_batch(0xffffffff)
        out_host = T.hash_to_group(eng, ts_host)
    finally:
        T.set_fused_min_batch(old)
    assert (out_dev == out_host).all() and (ts_dev == ts_host).all()


vrf_proof = T.define_proof("vrf_proof", b"VRF", ["x"], ["A", "G", "H"], ["B"], [("A", [("x", "B")]), ("G", [("x", "H")])])


def test_vrf_batch_from_product_calls(eng):
    """sig_and_vrf_example.rs's VRF for 4096 messages: H = hash_to_group(function transcript), G = x H (constant time), prove_compact on
    the proof transcripts, verify_compact -- then the example's reject cases (wrong pubkey, output, domain separator, message)."""
    rng = np.random.default_rng(13)
    n = 4096
    dom, other = b"My VRF Application", b"A different application"
    msgs = [b"Test Message %d" % j for j in range(n)]
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    x = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    x[:, 31] &= 0x0f
    iota = np.arange(n + 1, dtype=np.uint32)
    A, st = eng.msm_many(iota, x, np.zeros(n, np.uint32), B, ZKP_CT)
    assert not st.any()
    H = T.hash_to_group(eng, _function_transcripts(msgs, dom))
    G, st = eng.msm_many(iota, x, np.arange(n, dtype=np.uint32), H, ZKP_CT)
    assert not st.any()
    inst = np.ascontiguousarray(np.stack([A, G, H]))
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    ts = np.stack([T.Transcript(dom).state] * n)
    chal, resp, _ = T.prove_batch(eng, vrf_proof.statement, ts, x.reshape(n, 1, 32), inst, B, entropy)

    def verify(msgs_v, A_v, G_v, dom_v):
        H_v = T.hash_to_group(eng, _function_transcripts(msgs_v, dom))
        ts_v = np.stack([T.Transcript(dom_v).state] * n)
        return T.verify_compact_batch(eng, vrf_proof.statement, ts_v, np.ascontiguousarray(np.stack([A_v, G_v, H_v])), B, chal, resp)

    assert not verify(msgs, A, G, dom).any()
    bad = np.zeros(n, bool)
    bad[rng.choice(n, size=64, replace=False)] = True
    swap = np.where(bad, np.roll(np.arange(n), 1), np.arange(n))
    assert (verify(msgs, A[swap], G, dom) == bad).all()                                    # wrong pubkey
    assert (verify(msgs, A, G[swap], dom) == bad).all()                                    # wrong output
    assert verify(msgs, A, G, other).all()                                                 # wrong domain separator
    assert (verify([msgs[(j + 1) % n] if bad[j] else msgs[j] for j in range(n)], A, G, dom) == bad).all()   # wrong message
    # a sample against the oracle: H by the model's merlin and map, the proof byte for byte from the oracle's prover
    cst = C.Statement(b"VRF", ["x"], [("A", False), ("G", False), ("H", False), ("B", True)], [("A", [("x", "B")]), ("G", [("x", "H")])])
    want_h, _ = _model_hash([msgs[j] for j in range(0, n, 257)], dom)
    assert [bytes(H[j]) for j in range(0, n, 257)] == want_h
    for j in range(0, n, 257):
        assert bytes(G[j]) == M.ristretto_encode(M.pt_mul(int.from_bytes(x[j].tobytes(), "little"), M.ristretto_decode(bytes(H[j]))))
        ec, er, _, _ = C.prove(cst, dom, x[j].reshape(1, 32), np.stack([A[j], G[j], H[j], B[0]]), entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all()
        assert C.verify_compact(cst, dom, np.stack([A[j], G[j], H[j], B[0]]), chal[j], resp[j]) == 0

"""Batched Merlin operations on the MI355X: k_strobe_append_csr and k_strobe_challenge behind zkp_transcripts_append_message[_dev] and
zkp_transcripts_challenge_bytes[_dev], the toolbox routing, graph capture, and the transcripts they leave going into the fused flows.
Every result equals the host route (host Merlin on the host threads, which tests/test_host_transcript_ops.py holds against the oracle
model) byte for byte.  Inputs: tests/transcript_ops_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import model as M
from tests.test_gpu_device_entry import _cmz_fused_statement, _dev, _torch
from tests.test_gpu_ragged_transcripts import _sig
from tests.test_gpu_toolbox import _cmz_batch
from tests.transcript_ops_cases import LABELS, LC, LM, append_sweep, host_append, host_challenge, pos_word, start_states
from zkp_amd import toolbox as T
from zkp_amd.engine import messages_csr, strobe_pos_after_append

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2                                                                       # ZKP_ERR_ARG


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _dev_off(offsets):
    return _dev(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64))


@pytest.mark.parametrize("label", LABELS, ids=["empty", "msg", "200-bytes"])
def test_append_sweep_host_pointer_and_dev_forms(eng, label):
    """S x LM (6,327 transcripts in one call) through zkp_transcripts_append_message and through the _dev form, not shared, in place and out of place"""
    torch = _torch()
    ts, data, offsets = append_sweep()
    n = len(ts)
    want = host_append(ts, label, data, offsets)
    got = eng.transcripts_append_message(ts.copy(), label, data, offsets)
    assert (got == want).all()
    d_in, d_data, d_off = _dev(ts), _dev(data), _dev_off(offsets)
    d_out = torch.zeros((n + 2, 208), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_append_message_dev(n, 0, d_in.data_ptr(), d_out.data_ptr() + 208, label, d_data.data_ptr(), len(data), d_off.data_ptr())
    eng.synchronize()
    out = d_out.cpu().numpy()
    assert (out[1:n + 1] == want).all() and not out[0].any() and not out[n + 1].any()
    assert (d_in.cpu().numpy() == ts).all()
    eng.transcripts_append_message_dev(n, 0, d_in.data_ptr(), d_in.data_ptr(), label, d_data.data_ptr(), len(data), d_off.data_ptr())
    eng.synchronize()
    assert (d_in.cpu().numpy() == want).all()


@pytest.mark.parametrize("label", LABELS, ids=["empty", "msg", "200-bytes"])
def test_challenge_sweep_host_pointer_and_dev_forms(eng, label):
    """S x LC through both challenge_bytes forms: outputs and blobs.  S is repeated so that the call spans several wavefronts."""
    torch = _torch()
    S = np.repeat(start_states(), 3, axis=0)
    n = len(S)
    for k in LC:
        want_out, want_ts = host_challenge(S, label, k)
        ts = S.copy()
        assert (eng.transcripts_challenge_bytes(ts, label, k) == want_out).all() and (ts == want_ts).all(), k
        d_ts = _dev(S)
        d_out = torch.zeros(n * k + 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.transcripts_challenge_bytes_dev(n, d_ts.data_ptr(), label, k, d_out.data_ptr() + 3)        # outputs at an odd address
        eng.synchronize()
        out = d_out.cpu().numpy()
        assert (out[3:3 + n * k].reshape(n, k) == want_out).all() and not out[:3].any() and not out[3 + n * k:].any(), k
        assert (d_ts.cpu().numpy() == want_ts).all(), k


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_csr_edges(eng, n):
    """message data from an odd byte offset, runs of empty messages, one message of 100,000 bytes among short ones, the last message ending
    on the buffer's last byte; shared_initial = 1 equals n copies of the blob with shared_initial = 0"""
    rng = np.random.default_rng(n)
    lens = [int(k) for k in rng.integers(0, 40, size=n)]
    for j in range(3, n, 9):
        lens[j:j + 3] = [0] * len(lens[j:j + 3])
    lens[n // 2] = 100000
    lens[-1] = max(lens[-1], 1) if n > 1 else lens[-1]
    msgs = [rng.bytes(k) for k in lens]
    data, offsets = messages_csr(msgs)
    lead = 5
    data = np.concatenate([rng.integers(0, 256, size=lead, dtype=np.uint8), data[:int(offsets[-1])]])
    offsets = offsets + np.uint64(lead)
    assert int(offsets[-1]) == len(data) and int(offsets[0]) % 2 == 1
    S = start_states()
    ts = S[(np.arange(n) * 7) % 171]
    want = host_append(ts, b"msg", data, offsets)
    assert (eng.transcripts_append_message(ts.copy(), b"msg", data, offsets) == want).all()
    # the toolbox's device route, whatever host_max_terms says
    old = T.get_host_max_terms()
    T.set_host_max_terms(0)
    try:
        assert (T.append_messages_csr(ts.copy(), b"msg", data, offsets, eng=eng) == want).all()
    finally:
        T.set_host_max_terms(old)
    shared = np.concatenate([ts[:1], np.zeros((n - 1, 208), np.uint8)])
    got = eng.transcripts_append_message(shared, b"msg", data, offsets, shared_initial=True)
    assert (got == host_append(np.repeat(ts[:1], n, axis=0), b"msg", data, offsets)).all()
    # _dev, shared: one blob in, n blobs out, messages at an odd device address
    torch = _torch()
    d_one, d_data, d_off = _dev(ts[:1]), _dev(data), _dev_off(offsets - np.uint64(lead))
    d_out = torch.zeros((n, 208), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_append_message_dev(n, 1, d_one.data_ptr(), d_out.data_ptr(), b"msg", d_data.data_ptr() + lead, len(data) - lead, d_off.data_ptr())
    eng.synchronize()
    assert (d_out.cpu().numpy() == got).all()


def test_dev_form_clamps_ranges_and_passes_corrupt_blobs_through(eng):
    torch = _torch()
    rng = np.random.default_rng(9)
    data = rng.integers(0, 256, size=1000, dtype=np.uint8)
    S = start_states()
    n = 6
    ts = S[[0, 40, 80, 120, 160, 170]].copy()
    ts[4, 200] = 200                                                           # corrupt: position byte >= 166
    ts[4, 203:] = 0xee                                                         # ... comes back with every byte as it was
    #          in range     hi past the end    lo and hi past the end     hi < lo          corrupt         ends on the last byte
    ranges = [(10, 300), (900, 5000), (2000, 3000), (700, 100), (0, 50), (990, 1000)]
    clamped = [(10, 300), (900, 1000), (1000, 1000), (700, 700), (0, 50), (990, 1000)]
    offs = np.zeros((n, 2), np.uint64)
    want = ts.copy()
    for j, ((lo, hi), (clo, chi)) in enumerate(zip(ranges, clamped)):
        offs[j] = lo, hi
        if j != 4:
            want[j] = host_append(ts[j:j + 1], b"msg", data, np.array([clo, chi], np.uint64))[0]
    d_data = _dev(data)
    for j in range(n):                                                         # one call per range: d_offsets[j + 1] is the range's own end
        d_ts, d_off = _dev(ts[j:j + 1]), _dev_off(offs[j])
        torch.cuda.synchronize()
        eng.transcripts_append_message_dev(1, 0, d_ts.data_ptr(), d_ts.data_ptr(), b"msg", d_data.data_ptr(), len(data), d_off.data_ptr())
        eng.synchronize()
        assert (d_ts.cpu().numpy()[0] == want[j]).all(), j
    # challenge_bytes: the corrupt blob stays as it is and its output is zeros
    d_ts = _dev(ts)
    d_out = torch.full((n, 40), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_challenge_bytes_dev(n, d_ts.data_ptr(), b"c", 40, d_out.data_ptr())
    eng.synchronize()
    ok = [0, 1, 2, 3, 5]
    want_out, want_ts = host_challenge(ts[ok], b"c", 40)
    out, adv = d_out.cpu().numpy(), d_ts.cpu().numpy()
    assert (out[ok] == want_out).all() and (adv[ok] == want_ts).all()
    assert not out[4].any() and (adv[4] == ts[4]).all()


def test_argument_errors_change_nothing(eng):
    lib, p = eng._lib, (lambda x: x.ctypes.data)
    S = start_states()[:4]
    ts = S.copy()
    data = np.arange(40, dtype=np.uint8)
    ok = np.array([0, 10, 10, 25, 40], np.uint64)
    dec = np.array([0, 10, 5, 25, 40], np.uint64)
    out = np.zeros((4, 16), np.uint8)
    app, chal = lib.zkp_transcripts_append_message, lib.zkp_transcripts_challenge_bytes
    app_dev, chal_dev = lib.zkp_transcripts_append_message_dev, lib.zkp_transcripts_challenge_bytes_dev
    assert app(eng._h, 0, 0, None, b"msg", None, None) == 0 and chal(eng._h, 0, None, b"msg", 16, None) == 0
    assert app_dev(eng._h, 0, 0, None, None, b"msg", None, 0, None) == 0 and chal_dev(eng._h, 0, None, b"msg", 16, None) == 0
    assert app(None, 4, 0, p(ts), b"msg", p(data), p(ok)) == ARG and app(eng._h, 4, 0, p(ts), None, p(data), p(ok)) == ARG
    assert app(eng._h, 4, 0, None, b"msg", p(data), p(ok)) == ARG and app(eng._h, 4, 0, p(ts), b"msg", p(data), None) == ARG
    assert app(eng._h, 4, 0, p(ts), b"msg", None, p(ok)) == ARG and app(eng._h, 4, 0, p(ts), b"msg", p(data), p(dec)) == ARG
    assert app(eng._h, 4, 0, p(ts), 249 * b"x", p(data), p(ok)) == ARG
    assert chal(eng._h, 4, None, b"msg", 16, p(out)) == ARG and chal(eng._h, 4, p(ts), b"msg", 16, None) == ARG
    assert chal(eng._h, 4, p(ts), None, 16, p(out)) == ARG and chal(None, 4, p(ts), b"msg", 16, p(out)) == ARG
    bad = S.copy()
    bad[3, 200] = 166
    assert app(eng._h, 4, 0, p(bad), b"msg", p(data), p(ok)) == ARG and chal(eng._h, 4, p(bad), b"msg", 16, p(out)) == ARG
    assert (bad[:3] == S[:3]).all() and (ts == S).all() and not out.any()
    # _dev forms: NULL, alignment and overlap are checked before anything is queued
    assert app_dev(eng._h, 4, 0, None, 256, b"msg", 256, 40, 256) == ARG and app_dev(eng._h, 4, 0, 256, 256, None, 256, 40, 256) == ARG
    assert app_dev(eng._h, 4, 0, 264, 256, b"msg", 256, 40, 256) == ARG and app_dev(eng._h, 4, 0, 256, 256, b"msg", 256, 40, 260) == ARG
    assert app_dev(eng._h, 4, 0, 256, 256, b"msg", None, 40, 256) == ARG and app_dev(eng._h, 4, 1, 4096 + 208, 4096, b"msg", 256, 40, 256) == ARG
    assert chal_dev(eng._h, 4, 264, b"msg", 16, 256) == ARG and chal_dev(eng._h, 4, 256, b"msg", 16, None) == ARG
    # msgs may be NULL when every message is empty; len = 0 needs no output
    assert app(eng._h, 4, 0, p(ts), b"msg", None, p(np.zeros(5, np.uint64))) == 0
    assert (ts == host_append(S, b"msg", data, np.zeros(5, np.uint64))).all()
    ts = S.copy()
    assert chal(eng._h, 4, p(ts), b"msg", 0, None) == 0 and (ts == host_challenge(S, b"msg", 0)[1]).all()


def test_default_routing_and_kernel_names(eng):
    """host_max_terms at its default: N = 16 stays on the host threads, N = 17 runs the new kernels; same bytes"""
    before = T.get_host_max_terms()                                            # (the GPU tests run with 0: conftest.py)
    T.set_host_max_terms(16)                                                   # the default, g_host_max_terms of toolbox.cpp
    S = start_states()
    rng = np.random.default_rng(4)
    eng.set_profiling(True)
    try:
        for n, on_device in ((16, False), (17, True)):
            ts = S[40:40 + n]
            data, offsets = messages_csr([rng.bytes(150 + 3 * j) for j in range(n)])      # (short messages stay on the host threads at any N)
            eng.scalar_invert(np.ones((1, 32), np.uint8))                      # a call of another kind: the names below are this test's
            got = T.append_messages_csr(ts.copy(), b"msg", data, offsets, eng=eng)
            assert (got == host_append(ts, b"msg", data, offsets)).all()
            names = eng.last_kernels().get("transcript", [])
            assert ("zkp::k_strobe_append_csr" in names) == on_device, (n, names)
            if on_device:
                assert eng.last_timing()[0]["transcript"] > 0
            eng.scalar_invert(np.ones((1, 32), np.uint8))
            out = T.challenge_bytes(eng, got, b"c", 64)
            want_out, want_ts = host_challenge(host_append(ts, b"msg", data, offsets), b"c", 64)
            assert (out == want_out).all() and (got == want_ts).all()
            names = eng.last_kernels().get("transcript", [])
            assert ("zkp::k_strobe_challenge" in names) == on_device, (n, names)
        # messages of fewer than 128 bytes on average stay on the host threads: the device call loses there at every measured N
        data, offsets = messages_csr([rng.bytes(32) for _ in range(300)])
        ts = S[(np.arange(300) * 5) % 171]
        eng.scalar_invert(np.ones((1, 32), np.uint8))
        assert (T.append_messages_csr(ts.copy(), b"msg", data, offsets, eng=eng) == host_append(ts, b"msg", data, offsets)).all()
        assert "zkp::k_strobe_append_csr" not in eng.last_kernels().get("transcript", [])
    finally:
        eng.set_profiling(False)
        T.set_host_max_terms(before)


def test_recorded_append_then_challenge_replays_to_the_direct_calls(eng):
    torch = _torch()
    from zkp_amd.engine import Engine
    n = 300
    rng = np.random.default_rng(12)
    S = start_states()
    ts = S[(np.arange(n) * 11) % 171]
    data_a, offsets = messages_csr([rng.bytes(int(k)) for k in rng.integers(0, 400, size=n)])
    data_b = rng.integers(0, 256, size=len(data_a), dtype=np.uint8)
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_in, d_data, d_off = _dev(ts), _dev(data_a), _dev_off(offsets)
    d_ts = torch.zeros((n, 208), dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros((n, 64), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with e.capture() as cap:                                                   # no workspace: recorded without a warm-up call
        e.transcripts_append_message_dev(n, 0, d_in.data_ptr(), d_ts.data_ptr(), b"msg", d_data.data_ptr(), len(data_a), d_off.data_ptr())
        e.transcripts_challenge_bytes_dev(n, d_ts.data_ptr(), b"c", 64, d_out.data_ptr())
    assert not bool(d_ts.any().item()) and not bool(d_out.any().item())       # recorded, not run
    for data in (data_a, data_b):                                              # the replay follows new message bytes in the same buffer
        d_data.copy_(torch.from_numpy(data).to("cuda:0"))
        torch.cuda.synchronize()
        cap.graph.launch()
        e.synchronize()
        want_out, want_ts = host_challenge(host_append(ts, b"msg", data, offsets), b"c", 64)
        assert (d_out.cpu().numpy() == want_out).all() and (d_ts.cpu().numpy() == want_ts).all()
    cap.graph.close()
    e.close()


def _model_verify(st, label, msg, j, inst, common, coms, resp, weight):
    """proof j on Transcript::new(label) + append_message(b"msg", msg) through the oracle model's verifier; raises when it rejects"""
    t = M.Transcript(label)
    t.append_message(b"msg", msg)
    v = M.Verifier(st.proof_label, t)
    sv = [v.allocate_scalar(name) for name in st.secrets]
    pv, ki, kc = [], 0, 0
    for name, is_common in st.points:
        enc = common[kc] if is_common else inst[ki, j]
        kc, ki = kc + is_common, ki + (not is_common)
        pv.append(v.allocate_point(name, enc.tobytes()))
    for lhs, lc in st.constraints:
        v.constrain(pv[lhs], [(sv[s_], pv[p_]) for s_, p_ in lc])
    v.verify_batchable(M.BatchableProof([c.tobytes() for c in coms[j]], [int.from_bytes(r.tobytes(), "little") for r in resp[j]]), [weight] * len(st.constraints))


def test_signatures_on_device_appended_transcripts(eng):
    """257 signatures over messages of 8..599 bytes: append_messages(eng=eng) + prove_batch = the run with eng=None; the oracle accepts
    sampled proofs; the batch verifies, and fails when every message is swapped with its neighbour's.
    (The C oracle's verifier takes a transcript label only, not a transcript with a message in it: the sampled proofs go through
    oracle/model.py's Verifier, the Python restatement of the same reference code.)"""
    n = 257
    st, x, inst, common = _sig(n, 31)
    rng = np.random.default_rng(32)
    msgs = [rng.bytes(int(k)) for k in rng.integers(8, 600, size=n)]
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    label = b"My Sig Application"
    ts_host = T.append_messages(label, b"msg", msgs)
    ts_dev = T.append_messages(label, b"msg", msgs, eng=eng)
    assert (ts_dev == ts_host).all()
    chal_h, resp_h, coms_h = T.prove_batch(eng, st, ts_host, x, inst, common, entropy)
    chal, resp, coms = T.prove_batch(eng, st, ts_dev, x, inst, common, entropy)
    assert (chal == chal_h).all() and (resp == resp_h).all() and (coms == coms_h).all() and (ts_dev[:, :203] == ts_host[:, :203]).all()
    for j in [int(i) for i in rng.choice(n, size=64, replace=False)]:
        _model_verify(st, label, msgs[j], j, inst, common, coms, resp, 0x1234567 + j)
    T.batch_verify(eng, st, T.append_messages(label, b"msg", msgs, eng=eng), inst, common, coms, resp)
    with pytest.raises(T.VerificationFailure):
        T.batch_verify(eng, st, T.append_messages(label, b"msg", msgs[1:] + msgs[:1], eng=eng), inst, common, coms, resp)


def test_resident_append_feeds_fused_prove_dev(eng):
    """messages of one length through append_dev, then zkp_fused_prove_dev with the strobe_pos of zkp_strobe_pos_after_append: no blob is
    downloaded in between.  Equals the host-pointer run."""
    torch = _torch()
    n, mlen = 300, 45
    mod, secrets, inst, common = _cmz_batch(n, 23)
    fst = _cmz_fused_statement()
    rng = np.random.default_rng(24)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    msgs = rng.integers(0, 256, size=(n, mlen), dtype=np.uint8)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen)
    t0 = T.Transcript(b"resident").state
    ts = host_append(t0[None], b"msg", msgs.reshape(-1), offsets, shared=True)
    pos = strobe_pos_after_append(pos_word(t0), 3, mlen)
    assert {pos_word(b) for b in ts} == {pos}
    T.set_fused_min_batch(0)
    try:
        chal, resp, coms = T.prove_batch(eng, mod.statement, ts, secrets, inst, common, entropy)
    finally:
        T.set_fused_min_batch(32)
    eng.prepare_fixed_points(common)
    table = np.concatenate([common, inst.reshape(-1, 32)])
    d_t0, d_msgs, d_off = _dev(t0[None]), _dev(msgs), _dev_off(offsets)
    d_sec, d_tbl, d_ent = _dev(secrets), _dev(table), _dev(entropy)
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")        # noqa: E731
    d_ts, d_chal, d_resp, d_coms, d_st = z(n, 208), z(n, 32), z(n, 21, 32), z(n, 11, 32), z(11 * n)
    torch.cuda.synchronize()
    eng.transcripts_append_message_dev(n, 1, d_t0.data_ptr(), d_ts.data_ptr(), b"msg", d_msgs.data_ptr(), n * mlen, d_off.data_ptr())
    eng.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                        d_coms.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    assert not d_st.cpu().numpy().any()
    assert (d_chal.cpu().numpy() == chal).all() and (d_resp.cpu().numpy() == resp).all() and (d_coms.cpu().numpy() == coms).all()
    assert (d_ts.cpu().numpy()[:, :203] == ts[:, :203]).all()


def test_sig_chain_example_runs_as_a_child_process():
    """examples/sig_chain_batch.py 257: six rounds of ragged appends on both parties' transcripts, which end equal"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "sig_chain_batch.py"), "257"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "transcripts equal" in r.stdout

"""The witness RNG, challenge scalars and point appends on the MI355X: k_strobe_witness_rng, k_strobe_challenge_scalars and
k_strobe_append_points behind their host-pointer and _dev entry points, the toolbox routing, graph capture, and the transcripts they leave
going into the fused prover.  Every result equals the host route (the same lane code on the host threads, which
tests/test_host_transcript_rng.py holds against the oracle model and host Merlin) byte for byte.  Inputs: tests/transcript_rng_cases.py.
The host-pointer witness RNG's promise to zero its staging of entropy and witnesses is read back from the workspace (zkp_debug_ws_count)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_device_entry import _cmz_fused_statement, _dev, _torch
from tests.test_gpu_toolbox import _cmz_batch
from tests.transcript_ops_cases import host_challenge, pos_word
from tests.transcript_rng_cases import (BYTE_COUNTS, KINDS, LABELS, SCALAR_COUNTS, W, entropy, host_rng, points, start_states, tiled_states, witnesses)
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_RNG_BYTES, ZKP_RNG_SCALARS, strobe_pos_after_append

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -2                                                                       # ZKP_ERR_ARG
NEVER = 2**32 - 1
GRID_LANES = 2048 * 64                                                         # what the launcher's capped grid covers in one pass
MODES = [(ZKP_RNG_SCALARS, c) for c in SCALAR_COUNTS] + [(ZKP_RNG_BYTES, c) for c in BYTE_COUNTS]


@pytest.fixture(scope="module")
def eng():
    from zkp_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _odd(a, lead=3):
    """a on the device behind `lead` bytes: (tensor, pointer to the copy of a) -- buffers other than the blobs may have any alignment"""
    torch = _torch()
    flat = np.ascontiguousarray(a, np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(lead, 0xaa, np.uint8), flat, np.full(5, 0xaa, np.uint8)])).to("cuda:0")
    return t, t.data_ptr() + lead


def host_points(S, kind, label, pts, validate):
    ts = S.copy()
    f = T.append_point_vars if kind == b"ptvar" else T.append_blinding_commitments
    return f(None, ts, label, pts, validate=validate), ts


@pytest.mark.parametrize("shape", W, ids=["%dx%d" % s for s in W])
def test_witness_rng_host_pointer_and_dev_forms(eng, shape):
    """one call per (shape, label, count) over the 171 states: the lanes of a wavefront stand at different positions"""
    torch = _torch()
    m, wlen = shape
    S = start_states()
    wit, ent = witnesses(171, m, wlen), entropy(171)
    d_ts, (d_wit_t, d_wit), (d_ent_t, d_ent) = _dev(S), _odd(wit), _odd(ent, 1)
    for label in LABELS:
        for mode, count in MODES:
            want = host_rng(m, wlen, label, mode, count)
            ts = S.copy()
            got = eng.transcripts_witness_rng(ts, label, wit, ent, mode, count)
            assert (got == want).all() and (ts == S).all(), (label[:2], mode, count)
            row = want[0].size
            d_out = torch.full((171 * row + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.transcripts_witness_rng_dev(171, d_ts.data_ptr(), label, m, wlen, d_wit if m * wlen else None, d_ent, mode, count, d_out.data_ptr() + 3)
            eng.synchronize()
            out = d_out.cpu().numpy()
            assert (out[3:3 + 171 * row] == want.reshape(-1)).all() and (out[:3] == 0x55).all() and (out[3 + 171 * row:] == 0x55).all(), (label[:2], mode, count)
    assert (d_ts.cpu().numpy() == S).all()                                    # build_rng clones: the inputs are bit-identical


@pytest.mark.parametrize("label", LABELS, ids=["empty", "w", "200-bytes"])
def test_challenge_scalars_and_point_appends_host_pointer_and_dev_forms(eng, label):
    torch = _torch()
    S = np.repeat(start_states(), 3, axis=0)
    n = len(S)
    wide, want_ts = host_challenge(S, label, 64)
    want = T.scalar_from_wide(None, wide)
    assert (T.challenge_scalars(None, S.copy(), label) == want).all()
    ts = S.copy()
    assert (eng.transcripts_challenge_scalars(ts, label) == want).all() and (ts == want_ts).all()
    d_ts, d_out = _dev(S), torch.full((32 * n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_challenge_scalars_dev(n, d_ts.data_ptr(), label, d_out.data_ptr() + 3)
    eng.synchronize()
    out = d_out.cpu().numpy()
    assert (out[3:3 + 32 * n].reshape(n, 32) == want).all() and (out[:3] == 0x55).all() and (out[3 + 32 * n:] == 0x55).all()
    assert (d_ts.cpu().numpy() == want_ts).all()
    # the appends: `label` names the variable; rows of zeros among the points
    zero = [0, 1, 63, 64, 65, 200, n - 1]
    pts = points(n, zero)
    (d_pts_t, d_pts) = _odd(pts)
    for kind in KINDS + [LABELS[2]]:
        for validate in (False, True):
            f = eng.transcripts_append_points
            if kind in KINDS:
                want_st, want_ts = host_points(S, kind, label, pts, validate)
            else:                                                              # any label works as the kind: against the host route's C call
                want_ts, want_st = S.copy(), np.zeros(n, np.uint8)
                rc = T.lib().zkp_transcripts_append_points_batch(None, T._p(want_ts), n, kind, label, T._p(pts), int(validate), 0, T._p(want_st))
                assert rc == 0
            assert np.flatnonzero(want_st).tolist() == (zero if validate else [])
            ts = S.copy()
            assert (f(ts, kind, label, pts, validate) == want_st).all() and (ts == want_ts).all(), (kind[:8], validate)
            d_ts = _dev(S)
            d_st = torch.full((n + 8,), 0x55, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.transcripts_append_points_dev(n, d_ts.data_ptr(), kind, label, d_pts, validate, d_st.data_ptr() + 3)
            eng.synchronize()
            st = d_st.cpu().numpy()
            assert (st[3:3 + n] == want_st).all() and (st[:3] == 0x55).all() and (st[3 + n:] == 0x55).all() and (d_ts.cpu().numpy() == want_ts).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 171, 20000, GRID_LANES + 1])
def test_batch_sizes_around_a_wavefront_and_past_the_grid(eng, n):
    """shape (1, 32): N around the 64 lanes of a workgroup, 20,000, and one transcript more than the capped grid covers in one pass"""
    S, wit, ent, pts = tiled_states(n), witnesses(n, 1, 32), entropy(n), points(n, [0, n - 1])
    assert (eng.transcripts_witness_rng(S, b"", wit, ent, ZKP_RNG_SCALARS, 2) == host_rng(1, 32, b"", ZKP_RNG_SCALARS, 2, n)).all()
    assert (eng.transcripts_witness_rng(S, b"", wit, ent, ZKP_RNG_BYTES, 64) == host_rng(1, 32, b"", ZKP_RNG_BYTES, 64, n)).all()
    a, b = S.copy(), S.copy()
    assert (eng.transcripts_challenge_scalars(a, b"chal") == T.challenge_scalars(None, b, b"chal")).all() and (a == b).all()
    a = S.copy()
    want_st, want_ts = host_points(S, b"ptvar", b"A", pts, True)
    assert (eng.transcripts_append_points(a, b"ptvar", b"A", pts, True) == want_st).all() and (a == want_ts).all()


def test_dev_forms_pass_corrupt_blobs_through_and_leave_rng_inputs_alone(eng):
    torch = _torch()
    S = start_states()
    n = 6
    ts = S[[0, 40, 80, 120, 160, 170]].copy()
    ts[4, 200] = 200                                                           # corrupt: position byte >= 166
    ts[4, 203:] = 0xee                                                         # ... stays with every byte as it was
    ok = [0, 1, 2, 3, 5]
    wit, ent, pts = witnesses(n, 3, 32), entropy(n), points(n, [1, 4])
    d_wit, d_ent, d_pts = _dev(wit), _dev(ent), _dev(pts)
    for mode, count, f in ((ZKP_RNG_SCALARS, 2, T.witness_rng_scalars), (ZKP_RNG_BYTES, 40, T.witness_rng_bytes)):
        d_ts = _dev(ts)
        d_out = torch.full((n, count * (32 if mode == ZKP_RNG_SCALARS else 1)), 0x55, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        eng.transcripts_witness_rng_dev(n, d_ts.data_ptr(), b"w", 3, 32, d_wit.data_ptr(), d_ent.data_ptr(), mode, count, d_out.data_ptr())
        eng.synchronize()
        out = d_out.cpu().numpy()
        assert (out[ok] == f(None, ts[ok], wit[ok], count, ent[ok], b"w").reshape(5, -1)).all() and not out[4].any()
        assert (d_ts.cpu().numpy() == ts).all()                                # nothing of the inputs changes, the corrupt blob included
    d_ts = _dev(ts)
    d_out = torch.full((n, 32), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_challenge_scalars_dev(n, d_ts.data_ptr(), b"c", d_out.data_ptr())
    eng.synchronize()
    adv_want = ts[ok].copy()
    want = T.challenge_scalars(None, adv_want, b"c")
    out, adv = d_out.cpu().numpy(), d_ts.cpu().numpy()
    assert (out[ok] == want).all() and (adv[ok] == adv_want).all() and not out[4].any() and (adv[4] == ts[4]).all()
    d_ts = _dev(ts)
    d_st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.transcripts_append_points_dev(n, d_ts.data_ptr(), b"ptvar", b"A", d_pts.data_ptr(), True, d_st.data_ptr())
    eng.synchronize()
    want_st, want_ts = host_points(ts[ok], b"ptvar", b"A", pts[ok], True)
    st, adv = d_st.cpu().numpy(), d_ts.cpu().numpy()
    assert (st[ok] == want_st).all() and st[1] == 1 and st[4] == 0 and (adv[ok] == want_ts).all() and (adv[4] == ts[4]).all()
    # without validation the status buffer may be missing
    d_ts = _dev(ts[ok])
    torch.cuda.synchronize()
    eng.transcripts_append_points_dev(5, d_ts.data_ptr(), b"blindcom", b"A", d_pts.data_ptr(), False, None)
    eng.synchronize()
    assert (d_ts.cpu().numpy() == host_points(ts[ok], b"blindcom", b"A", pts[:5], False)[1]).all()


def test_argument_errors_change_nothing(eng):
    lib, p, h = eng._lib, (lambda x: x.ctypes.data), eng._h
    S = start_states()[:4]
    ts, wit, ent, pts = S.copy(), witnesses(4, 1, 32), entropy(4), points(4)
    out, sc, st = np.zeros((4, 2, 32), np.uint8), np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    long_label = 249 * b"x"
    rng_, chal, app = lib.zkp_transcripts_witness_rng, lib.zkp_transcripts_challenge_scalars, lib.zkp_transcripts_append_points
    rng_dev, chal_dev, app_dev = lib.zkp_transcripts_witness_rng_dev, lib.zkp_transcripts_challenge_scalars_dev, lib.zkp_transcripts_append_points_dev
    assert rng_(h, 0, None, b"", 1, 32, None, None, 0, 2, None) == 0 and chal(h, 0, None, b"c", None) == 0 and app(h, 0, None, b"ptvar", b"A", None, 1, None) == 0
    assert rng_dev(h, 0, None, b"", 1, 32, None, None, 0, 2, None) == 0 and chal_dev(h, 0, None, b"c", None) == 0
    assert app_dev(h, 0, None, b"ptvar", b"A", None, 1, None) == 0
    good = dict(ts=p(ts), label=b"", wit=p(wit), ent=p(ent), mode=0, out=p(out))
    for change in (dict(ts=None), dict(label=None), dict(label=long_label), dict(wit=None), dict(ent=None), dict(mode=2), dict(out=None)):
        a = dict(good, **change)
        assert rng_(h, 4, a["ts"], a["label"], 1, 32, a["wit"], a["ent"], a["mode"], 2, a["out"]) == ARG, change
    assert rng_(None, 4, p(ts), b"", 1, 32, p(wit), p(ent), 0, 2, p(out)) == ARG
    assert chal(h, 4, None, b"c", p(sc)) == ARG and chal(h, 4, p(ts), None, p(sc)) == ARG and chal(h, 4, p(ts), b"c", None) == ARG
    assert chal(h, 4, p(ts), long_label, p(sc)) == ARG and chal(None, 4, p(ts), b"c", p(sc)) == ARG
    assert app(h, 4, None, b"ptvar", b"A", p(pts), 1, p(st)) == ARG and app(h, 4, p(ts), None, b"A", p(pts), 1, p(st)) == ARG
    assert app(h, 4, p(ts), b"ptvar", None, p(pts), 1, p(st)) == ARG and app(h, 4, p(ts), b"ptvar", b"A", None, 1, p(st)) == ARG
    assert app(h, 4, p(ts), b"ptvar", b"A", p(pts), 1, None) == ARG and app(h, 4, p(ts), long_label, b"A", p(pts), 1, p(st)) == ARG
    assert app(h, 4, p(ts), b"ptvar", long_label, p(pts), 1, p(st)) == ARG and app(None, 4, p(ts), b"ptvar", b"A", p(pts), 1, p(st)) == ARG
    bad = S.copy()
    bad[3, 200] = 166
    assert rng_(h, 4, p(bad), b"", 1, 32, p(wit), p(ent), 0, 2, p(out)) == ARG and chal(h, 4, p(bad), b"c", p(sc)) == ARG
    assert app(h, 4, p(bad), b"ptvar", b"A", p(pts), 1, p(st)) == ARG
    assert (bad[:3] == S[:3]).all() and (ts == S).all() and not out.any() and not sc.any() and not st.any()
    # _dev forms: NULL and alignment are checked before anything is queued
    assert rng_dev(h, 4, None, b"", 1, 32, 256, 256, 0, 2, 256) == ARG and rng_dev(h, 4, 264, b"", 1, 32, 256, 256, 0, 2, 256) == ARG
    assert rng_dev(h, 4, 256, b"", 1, 32, None, 256, 0, 2, 256) == ARG and rng_dev(h, 4, 256, b"", 1, 32, 256, None, 0, 2, 256) == ARG
    assert rng_dev(h, 4, 256, b"", 1, 32, 256, 256, 0, 2, None) == ARG and rng_dev(h, 4, 256, long_label, 1, 32, 256, 256, 0, 2, 256) == ARG
    assert rng_dev(h, 4, 256, b"", 1, 32, 256, 256, 7, 2, 256) == ARG
    assert chal_dev(h, 4, 264, b"c", 256) == ARG and chal_dev(h, 4, 256, b"c", None) == ARG and chal_dev(h, 4, None, b"c", 256) == ARG
    assert app_dev(h, 4, 264, b"ptvar", b"A", 256, 0, None) == ARG and app_dev(h, 4, 256, b"ptvar", b"A", None, 0, None) == ARG
    assert app_dev(h, 4, 256, b"ptvar", b"A", 256, 1, None) == ARG
    # what may be NULL
    assert rng_(h, 4, p(ts), b"", 0, 32, None, p(ent), 0, 2, p(out)) == 0 and (out == host_rng(0, 0, b"", 0, 2)[:4]).all()
    assert rng_(h, 4, p(ts), b"", 1, 0, None, p(ent), 1, 0, None) == 0 and (ts == S).all()
    assert app(h, 4, p(ts), b"ptvar", b"A", p(pts), 0, None) == 0 and (ts == host_points(S, b"ptvar", b"A", pts, False)[1]).all()


def test_default_routing_and_kernel_names(eng):
    """The defaults of zkp_toolbox_get_*_min_batch follow profiles/transcript_rng_bench.txt.  A call just below its minimum batch stays on the
    host threads (none of the new kernels' names in zkp_ctx_last_kernels), a call at it runs the new kernel; `never` has no such batch, so
    the largest batch here stays on the host and an explicit minimum is what routes to the device.  Same bytes everywhere."""
    getters = (T.get_witness_rng_min_batch, T.get_challenge_scalars_min_batch, T.get_append_points_min_batch)
    big = max([4096] + [g() for g in getters if g() != NEVER])
    assert big <= 2**20
    S = tiled_states(big)
    wit, ent, pts = witnesses(big, 1, 32), entropy(big), points(big)
    calls = (("zkp::k_strobe_witness_rng", T.get_witness_rng_min_batch, T.set_witness_rng_min_batch,
              lambda e, n: T.witness_rng_scalars(e, S[:n], wit[:n], 1, ent[:n])),
             ("zkp::k_strobe_challenge_scalars", T.get_challenge_scalars_min_batch, T.set_challenge_scalars_min_batch,
              lambda e, n: T.challenge_scalars(e, S[:n].copy(), b"chal")),
             ("zkp::k_strobe_append_points", T.get_append_points_min_batch, T.set_append_points_min_batch,
              lambda e, n: T.append_point_vars(e, S[:n].copy(), b"A", pts[:n], True)))
    eng.set_profiling(True)
    try:
        for name, get, set_, call in calls:
            default = get()
            routes = [(4096, False)] if default == NEVER else ([(default - 1, False)] if default > 1 else []) + [(default, True)]
            try:
                for n, on_device in routes + [(None, True)]:
                    if n is None:                                              # an explicit minimum: 65 transcripts run on the device at 65
                        set_(65)
                        n = 65
                        eng.scalar_invert(np.ones((1, 32), np.uint8))
                        assert (call(eng, 64) == call(None, 64)).all() and name not in eng.last_kernels().get("transcript", [])
                    eng.scalar_invert(np.ones((1, 32), np.uint8))             # a call of another kind: the names below are this test's
                    assert (call(eng, n) == call(None, n)).all()
                    names = eng.last_kernels().get("transcript", [])
                    assert (name in names) == on_device, (name, n, names)
                    if on_device:
                        assert eng.last_timing()[0]["transcript"] > 0
            finally:
                set_(default)
    finally:
        eng.set_profiling(False)


def test_recorded_append_rng_challenge_chain_replays_to_the_direct_calls(eng):
    torch = _torch()
    from zkp_amd.engine import Engine
    n = 300
    S = tiled_states(n)
    wit, ent = witnesses(n, 2, 32), entropy(n)
    pts_a, pts_b = points(n, [7]), points(n, [8])[::-1].copy()
    e = Engine(0)
    stream = torch.cuda.Stream()
    e.set_stream(stream.cuda_stream)
    d_ts, d_pts, d_wit, d_ent = _dev(S), _dev(pts_a), _dev(wit), _dev(ent)
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")        # noqa: E731
    d_st, d_nonce, d_chal = z(n), z(n, 3, 32), z(n, 32)
    torch.cuda.synchronize()
    with e.capture() as cap:                                                   # no workspace: recorded without a warm-up call
        e.transcripts_append_points_dev(n, d_ts.data_ptr(), b"ptvar", b"A", d_pts.data_ptr(), True, d_st.data_ptr())
        e.transcripts_witness_rng_dev(n, d_ts.data_ptr(), b"", 2, 32, d_wit.data_ptr(), d_ent.data_ptr(), ZKP_RNG_SCALARS, 3, d_nonce.data_ptr())
        e.transcripts_challenge_scalars_dev(n, d_ts.data_ptr(), b"chal", d_chal.data_ptr())
    assert (d_ts.cpu().numpy() == S).all() and not bool(d_nonce.any().item()) and not bool(d_chal.any().item())       # recorded, not run
    for pts in (pts_a, pts_b):                                                 # the replay follows new points and fresh blobs in the same buffers
        d_pts.copy_(torch.from_numpy(pts).to("cuda:0"))
        d_ts.copy_(torch.from_numpy(S).to("cuda:0"))
        torch.cuda.synchronize()
        cap.graph.launch()
        e.synchronize()
        want_st, ts = host_points(S, b"ptvar", b"A", pts, True)
        want_nonce = T.witness_rng_scalars(None, ts, wit, 3, ent)
        want_chal = T.challenge_scalars(None, ts, b"chal")
        assert (d_st.cpu().numpy() == want_st).all() and (d_nonce.cpu().numpy() == want_nonce).all()
        assert (d_chal.cpu().numpy() == want_chal).all() and (d_ts.cpu().numpy() == ts).all()
    cap.graph.close()
    e.close()


def test_device_appended_points_feed_fused_prove_dev_and_verify(eng):
    """a per-proof point bound into each transcript by append_point_vars on the device, then zkp_fused_prove_dev at the position that
    zkp_strobe_pos_after_append gives for the two appends: no blob is downloaded in between.  Equals the host run, and the proofs verify."""
    torch = _torch()
    n = 300
    mod, secrets, inst, common = _cmz_batch(n, 23)
    fst = _cmz_fused_statement()
    ent = np.random.default_rng(24).integers(0, 256, size=(n, 32), dtype=np.uint8)
    pts = points(n)
    t0 = np.stack([T.Transcript(b"resident").state] * n)
    ts = t0.copy()
    assert not T.append_point_vars(None, ts, b"holder", pts, validate=True).any()
    pos = strobe_pos_after_append(strobe_pos_after_append(pos_word(t0[0]), 5, 6), 3, 32)
    assert {pos_word(b) for b in ts} == {pos}
    bound = ts.copy()
    T.set_fused_min_batch(0)
    try:
        chal, resp, coms = T.prove_batch(eng, mod.statement, ts, secrets, inst, common, ent)
        assert not T.verify_compact_batch(eng, mod.statement, bound.copy(), inst, common, chal, resp).any()
    finally:
        T.set_fused_min_batch(32)
    eng.prepare_fixed_points(common)
    table = np.concatenate([common, inst.reshape(-1, 32)])
    d_ts, d_pts, d_sec, d_tbl, d_ent = _dev(t0), _dev(pts), _dev(secrets), _dev(table), _dev(ent)
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")        # noqa: E731
    d_chal, d_resp, d_coms, d_st, d_rej = z(n, 32), z(n, 21, 32), z(n, 11, 32), z(11 * n), z(n)
    torch.cuda.synchronize()
    eng.transcripts_append_points_dev(n, d_ts.data_ptr(), b"ptvar", b"holder", d_pts.data_ptr(), True, d_rej.data_ptr())
    eng.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                        d_coms.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    assert not d_st.cpu().numpy().any() and not d_rej.cpu().numpy().any()
    assert (d_chal.cpu().numpy() == chal).all() and (d_resp.cpu().numpy() == resp).all() and (d_coms.cpu().numpy() == coms).all()
    assert (d_ts.cpu().numpy()[:, :203] == ts[:, :203]).all()


def _windows_found(e, rows, offsets=(0, 16)):
    """(row, offset) of every 16-byte window of `rows` that occurs somewhere in the workspace of e"""
    return [(i, o) for i, r in enumerate(rows) for o in offsets if e.debug_ws_count(r[o:o + 16].tobytes())]


@pytest.mark.parametrize("mode,count", ((ZKP_RNG_SCALARS, 2), (ZKP_RNG_BYTES, 64)), ids=("scalars", "bytes"))
def test_witness_rng_wipes_its_staging_of_entropy_and_witnesses_and_not_the_outputs(mode, count):
    """include/zkp_mi355x.h, zkp_transcripts_witness_rng (host-pointer form): the staging of entropy and witnesses is zeroed on every way out,
    the outputs' staging is not.  Read back with zkp_debug_ws_count (test-hook build): after the call no half of any witness or entropy row is
    in the workspace, while output rows are (the control: a search of the wrong place finds neither), and a fill with zeros removes those too.
    The success path is the only way out that valid arguments reach once secrets are on the device: after the uploads the call can fail only
    where the HIP runtime does."""
    from zkp_amd.engine import Engine, ZkpError
    n, m, wlen = 65, 2, 32
    rng = np.random.default_rng(4656 + mode)
    S = tiled_states(n)
    wit = rng.integers(0, 256, size=(n, m, wlen), dtype=np.uint8)
    ent = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    secret_rows = np.concatenate([wit.reshape(-1, wlen), ent])
    f = T.witness_rng_scalars if mode == ZKP_RNG_SCALARS else T.witness_rng_bytes
    want = f(None, S, wit, count, ent, b"w")
    e = Engine(0, test_hooks=True)
    try:
        assert e.debug_ws_count(bytes(16)) == 0                                # no workspace yet
        got = e.transcripts_witness_rng(S.copy(), b"w", wit, ent, mode, count)
        assert (got == want).all()
        assert e.debug_ws_bytes() >= 208 * n + secret_rows.size + got.size
        assert _windows_found(e, secret_rows) == []
        out_rows = got.reshape(n, -1)
        assert len(_windows_found(e, out_rows, (0,))) == n                     # every output row is still there ...
        assert e.debug_ws_count(bytes(16)) >= 1                                # ... and zeros stand where the secrets stood
        e.debug_fill_workspace(0, 0)
        assert _windows_found(e, out_rows, (0,)) == []
        e.capture_begin()
        try:
            with pytest.raises(ZkpError):
                e.debug_ws_count(bytes(16))
        finally:
            e.capture_abort()
    finally:
        e.close()


def test_or_ballot_example_runs_as_a_child_process():
    """examples/or_ballot_batch.py 4096 on the device: every ballot accepted, both bad ballots rejected, the tally right"""
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "examples", "or_ballot_batch.py"), "4096"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "ballots verified: 4096 of 4096" in lines and "m = 2 ballot: rejected" in lines and "swapped c_0 ballot: rejected" in lines
    cast = int(np.random.default_rng(4096).integers(0, 2, size=4096).sum())
    assert "tally: %d yes of 4096 (cast: %d)" % (cast, cast) in lines

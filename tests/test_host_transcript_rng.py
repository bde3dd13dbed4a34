"""The batched witness RNG, challenge scalars and point appends without a GPU: the toolbox's host route (ctx == NULL, the lane code of
zkp_amd/csrc/strobe_lane.h on host threads) against oracle/model.py's TranscriptRng and the calls it extends, whole proofs rebuilt from
the public calls against the product's prover, the lane code under AddressSanitizer and UBSan in a stand-alone program against host
Merlin, and the OR-ballot example.  Inputs: tests/transcript_rng_cases.py."""
import os
import shutil
import subprocess
import sys

import numpy as np

from oracle import model as M
from tests.transcript_ops_cases import host_append, host_challenge
from tests.transcript_rng_cases import (BYTE_COUNTS, EIGHT, KINDS, LABELS, RATE, SCALAR_COUNTS, W, entropy, host_rng, points, start_states, state_at,
                                        witnesses)
from zkp_amd import toolbox as T
from zkp_amd.engine import messages_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BAD = -10          # ZKP_TB_BAD_STATEMENT
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


def model_transcript(blob) -> M.Transcript:
    t = M.Transcript(b"x")
    s = t.strobe
    s.state[:] = bytes(blob[:200])
    s.pos, s.pos_begin, s.cur_flags = int(blob[200]), int(blob[201]), int(blob[202])
    return t


def model_rng(blob, label: bytes, wit, ent) -> M.TranscriptRng:
    b = model_transcript(blob).build_rng()
    for w in wit:
        b.rekey_with_witness_bytes(label, bytes(w))
    return b.finalize(bytes(ent))


def model_outputs(rng: M.TranscriptRng, mode: int, count: int) -> bytes:
    """the outputs of a COPY of rng (the builder's work is shared by every count)"""
    r = M.TranscriptRng(rng.strobe.clone())
    if mode == T.RNG_SCALARS:
        return b"".join(M.sc_to_bytes(r.random_scalar()) for _ in range(count))
    return r.fill_bytes(count)


def test_cases_are_the_ones_the_header_names():
    S = start_states()
    assert S.shape == (171, 208) and {int(b[200]) for b in S} == set(range(RATE))
    assert len(W) == 10 and SCALAR_COUNTS == [1, 2, 5] and BYTE_COUNTS == [0, 1, 64, 165, 166, 167, 400] and [len(x) for x in LABELS] == [0, 1, 200]
    assert [int(S[state_at(p)][200]) for p in EIGHT] == EIGHT and len(EIGHT) == 8


def test_witness_rng_equals_the_model_on_every_state():
    """all 171 states, shape (1, 32), label "": two scalars and 64 bytes"""
    S, wit, ent = start_states(), witnesses(171, 1, 32), entropy(171)
    sc, by = host_rng(1, 32, b"", T.RNG_SCALARS, 2), host_rng(1, 32, b"", T.RNG_BYTES, 64)
    assert (S == start_states()).all()
    for j in range(171):
        rng = model_rng(S[j], b"", wit[j], ent[j])
        assert sc[j].tobytes() == model_outputs(rng, T.RNG_SCALARS, 2), j
        assert by[j].tobytes() == model_outputs(rng, T.RNG_BYTES, 64), j


def test_witness_rng_equals_the_model_for_every_shape_label_and_count():
    """W x labels x counts on the eight states of EIGHT; the model keys each (shape, label, state) once and clones for the counts"""
    S = start_states()
    rows = [state_at(p) for p in EIGHT]
    ent = entropy(171)
    for m, wlen in W:
        wit = witnesses(171, m, wlen)
        for label in LABELS:
            got = {(mode, c): host_rng(m, wlen, label, mode, c) for mode, counts in ((T.RNG_SCALARS, SCALAR_COUNTS), (T.RNG_BYTES, BYTE_COUNTS)) for c in counts}
            for j in rows:
                rng = model_rng(S[j], label, wit[j], ent[j])
                for (mode, c), out in got.items():
                    assert out[j].tobytes() == model_outputs(rng, mode, c), (m, wlen, label[:2], mode, c, j)
    # m = 0 and wlen = 0 are different transcripts
    assert (host_rng(0, 0, b"", T.RNG_SCALARS, 1) != host_rng(1, 0, b"", T.RNG_SCALARS, 1)).any(axis=(1, 2)).all()


def test_drawn_entropy_differs_from_call_to_call_and_given_entropy_does_not():
    S, wit = start_states(), witnesses(171, 1, 32)
    a, b = T.witness_rng_scalars(None, S, wit, 1), T.witness_rng_scalars(None, S, wit, 1)
    assert (a != b).any(axis=(1, 2)).all()
    assert (T.witness_rng_scalars(None, S, wit, 1, entropy(171)) == host_rng(1, 32, b"", T.RNG_SCALARS, 1)).all()
    assert (T.witness_rng_scalars(T.HostEngine(), S, wit, 1, entropy(171)) == host_rng(1, 32, b"", T.RNG_SCALARS, 1)).all()


def test_challenge_scalars_equal_challenge_bytes_then_from_wide():
    S = start_states()
    for label in LABELS + [b"chal"]:
        wide, adv = host_challenge(S, label, 64)
        ts = S.copy()
        got = T.challenge_scalars(None, ts, label)
        assert (got == T.scalar_from_wide(None, wide)).all() and (ts == adv).all(), label[:4]
    m = model_transcript(S[5])
    assert M.sc_to_bytes(m.get_challenge(b"chal")) == T.challenge_scalars(None, S[5:6].copy(), b"chal")[0].tobytes()


def two_appends(S, kind: bytes, label: bytes, pts):
    n = len(S)
    ts = host_append(S, kind, *messages_csr([label] * n))
    return host_append(ts, b"val", *messages_csr([bytes(p) for p in pts]))


def test_point_appends_equal_two_append_messages():
    S = start_states()
    pts = points(171)
    for f, kind in ((T.append_point_vars, KINDS[0]), (T.append_blinding_commitments, KINDS[1])):
        for label in LABELS + [b"C_1"]:
            want = two_appends(S, kind, label, pts)
            for validate in (False, True):
                ts = S.copy()
                status = f(None, ts, label, pts, validate=validate)
                assert not status.any() and (ts == want).all(), (kind, label[:4], validate)
    # the identity's encoding: refused only when validating; its neighbours advance
    zero = [0, 1, 63, 64, 100, 170]
    pz = points(171, zero)
    want = two_appends(S, b"ptvar", b"A", pz)
    ts = S.copy()
    status = T.append_point_vars(None, ts, b"A", pz, validate=True)
    assert np.flatnonzero(status).tolist() == zero and set(status.tolist()) == {0, 1}
    keep = np.setdiff1d(np.arange(171), zero)
    assert (ts[zero] == S[zero]).all() and (ts[keep] == want[keep]).all()
    ts = S.copy()
    assert not T.append_blinding_commitments(None, ts, b"A", pz, validate=False).any() and (ts == two_appends(S, b"blindcom", b"A", pz)).all()
    # domain_sep and append_scalar_var over append_messages, against the model
    ts = S[:3].copy()
    T.domain_sep(ts, b"DLEQ proof")
    T.append_scalar_vars(ts, b"x")
    for j in range(3):
        m = model_transcript(S[j])
        m.domain_sep(b"DLEQ proof")
        m.append_scalar_var(b"x")
        assert bytes(m.strobe.state) + bytes([m.strobe.pos, m.strobe.pos_begin, m.strobe.cur_flags]) + bytes(5) == ts[j].tobytes()


def rebuild_proofs(mod, n, secrets, inst, common, ent):
    """prover.rs:41-112 out of the public calls -> (blindings, challenges, responses, commitments)"""
    st = mod.statement
    ts = np.stack([T.Transcript(b"rebuilt").state] * n)
    T.domain_sep(ts, mod.label)
    for name in mod.secrets:
        T.append_scalar_vars(ts, name.encode())
    for i, name in enumerate(mod.instance):
        assert not T.append_point_vars(None, ts, name.encode(), inst[i]).any()
    for i, name in enumerate(mod.common):
        assert not T.append_point_vars(None, ts, name.encode(), np.tile(common[i], (n, 1))).any()
    blind = T.witness_rng_scalars(None, ts, secrets, st.m, ent)
    pv = {name: ("i", i) for i, name in enumerate(mod.instance)}
    pv.update({name: ("c", i) for i, name in enumerate(mod.common)})
    sv = {name: i for i, name in enumerate(mod.secrets)}
    table = np.concatenate([common, inst.reshape(-1, 32)])
    coms = []
    for lhs, lc in mod.constraints:
        off = np.arange(0, n * len(lc) + 1, len(lc), dtype=np.uint32)
        sc = np.ascontiguousarray(np.stack([blind[:, sv[s]] for s, _ in lc], axis=1)).reshape(-1, 32)
        pidx = np.stack([np.full(n, pv[p][1], np.uint32) if pv[p][0] == "c" else len(common) + pv[p][1] * n + np.arange(n, dtype=np.uint32) for _, p in lc],
                        axis=1).reshape(-1).astype(np.uint32)
        out, bad = T.multiscalar_mul(None, off, sc, pidx, table, 1)
        assert not bad.any()
        coms.append(out)
        T.append_blinding_commitments(None, ts, lhs.encode(), out)
    c = T.challenge_scalars(None, ts, b"chal")
    resp = np.stack([T.scalar_muladd(None, np.ascontiguousarray(secrets[:, i]), c, np.ascontiguousarray(blind[:, i])) for i in range(st.m)], axis=1)
    return blind, c, resp, np.stack(coms, axis=1), ts


def test_proofs_rebuilt_from_the_public_calls_are_the_products():
    rng = np.random.default_rng(11)
    for mod, n in ((T.dleq_module(), 40), (T.cmz_module(3), 9)):
        st = mod.statement
        secrets = rng.integers(0, 256, size=(n, st.m, 32), dtype=np.uint8)
        secrets[:, :, 31] &= 0x0f
        inst = T.basepoint_mul(None, rng.integers(0, 256, size=(st.ni * n, 32), dtype=np.uint8)).reshape(st.ni, n, 32)
        common = T.basepoint_mul(None, rng.integers(0, 256, size=(st.ns, 32), dtype=np.uint8))
        ent = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        blind, chal, resp, coms, ts = rebuild_proofs(mod, n, secrets, inst, common, ent)
        t0 = np.stack([T.Transcript(b"rebuilt").state] * n)
        want_blind = T.prove_phase_a(st, t0, secrets, inst, common, ent)[0]
        assert (blind == want_blind).all(), mod.name
        t1 = np.stack([T.Transcript(b"rebuilt").state] * n)
        wc, wr, wk = T.prove_batch(T.HostEngine(), st, t1, secrets, inst, common, ent)
        assert (chal == wc).all() and (resp == wr).all() and (coms == wk).all() and (ts == t1).all(), mod.name


def test_one_and_sixteen_threads_give_the_same_bytes():
    S = np.repeat(start_states(), 4, axis=0)
    n = len(S)
    wit, ent, pts = witnesses(n, 3, 32), entropy(n), points(n, [5])
    for mode, f, c in ((0, T.witness_rng_scalars, 2), (1, T.witness_rng_bytes, 167)):
        assert (f(None, S, wit, c, ent, b"w", threads=1) == f(None, S, wit, c, ent, b"w", threads=16)).all()
    a, b = S.copy(), S.copy()
    assert (T.challenge_scalars(None, a, b"chal", threads=1) == T.challenge_scalars(None, b, b"chal", threads=16)).all() and (a == b).all()
    a, b = S.copy(), S.copy()
    assert (T.append_point_vars(None, a, b"A", pts, True, threads=1) == T.append_point_vars(None, b, b"A", pts, True, threads=16)).all() and (a == b).all()


def test_no_ops_null_buffers_long_labels_and_bad_positions():
    lib, p = T.lib(), T._p
    rng_, chal, app = lib.zkp_transcripts_witness_rng_batch, lib.zkp_transcripts_challenge_scalars_batch, lib.zkp_transcripts_append_points_batch
    S = start_states()[:4]
    ts, wit, ent, pts = S.copy(), witnesses(4, 1, 32), entropy(4), points(4)
    out, sc, st = np.zeros((4, 2, 32), np.uint8), np.zeros((4, 32), np.uint8), np.zeros(4, np.uint8)
    long_label = bytes(249 * [97])
    assert rng_(None, None, 0, b"", 1, 32, None, None, 0, 2, 0, None) == 0 and chal(None, None, 0, b"c", 0, None) == 0
    assert app(None, None, 0, b"ptvar", b"A", None, 1, 0, None) == 0
    # NULL buffers, NULL and long labels, another mode
    for args in ((None, 4, b"", 1, 32, p(wit), p(ent), 0, 2, 0, p(out)), (p(ts), 4, None, 1, 32, p(wit), p(ent), 0, 2, 0, p(out)),
                 (p(ts), 4, b"", 1, 32, None, p(ent), 0, 2, 0, p(out)), (p(ts), 4, b"", 1, 32, p(wit), p(ent), 0, 2, 0, None),
                 (p(ts), 4, long_label, 1, 32, p(wit), p(ent), 0, 2, 0, p(out)), (p(ts), 4, b"", 1, 32, p(wit), p(ent), 2, 2, 0, p(out))):
        assert rng_(None, *args) == T_BAD
    for args in ((None, 4, b"c", 0, p(sc)), (p(ts), 4, None, 0, p(sc)), (p(ts), 4, b"c", 0, None), (p(ts), 4, long_label, 0, p(sc))):
        assert chal(None, *args) == T_BAD
    for args in ((None, 4, b"ptvar", b"A", p(pts), 1, 0, p(st)), (p(ts), 4, None, b"A", p(pts), 1, 0, p(st)), (p(ts), 4, b"ptvar", None, p(pts), 1, 0, p(st)),
                 (p(ts), 4, b"ptvar", b"A", None, 1, 0, p(st)), (p(ts), 4, b"ptvar", b"A", p(pts), 1, 0, None), (p(ts), 4, long_label, b"A", p(pts), 1, 0, p(st)),
                 (p(ts), 4, b"ptvar", long_label, p(pts), 1, 0, p(st))):
        assert app(None, *args) == T_BAD
    # a position byte of 166 or more is no STROBE state: refused before anything changes
    bad = S.copy()
    bad[2, 200] = RATE
    assert rng_(None, p(bad), 4, b"", 1, 32, p(wit), p(ent), 0, 2, 0, p(out)) == T_BAD and chal(None, p(bad), 4, b"c", 0, p(sc)) == T_BAD
    assert app(None, p(bad), 4, b"ptvar", b"A", p(pts), 1, 0, p(st)) == T_BAD
    assert (bad[[0, 1, 3]] == S[[0, 1, 3]]).all() and bad[2, 200] == RATE and (bad[2, :200] == S[2, :200]).all()
    assert (ts == S).all() and not out.any() and not sc.any() and not st.any()
    # what may be NULL: witnesses when m * wlen = 0, the output when count = 0, the status when not validating; a 248-byte label is fine
    assert (ent == entropy(171)[:4]).all()
    assert rng_(None, p(ts), 4, b"", 0, 32, None, p(ent), 0, 2, 0, p(out)) == 0 and (out == host_rng(0, 0, b"", 0, 2)[:4]).all()
    assert rng_(None, p(ts), 4, b"", 1, 0, None, p(ent), 1, 0, 0, None) == 0
    assert app(None, p(ts), 4, b"ptvar", b"A", p(pts), 0, 0, None) == 0 and (ts == two_appends(S, b"ptvar", b"A", pts)).all()
    assert chal(None, p(ts), 4, long_label[:248], 0, p(sc)) == 0 and sc.any()


def test_routing_defaults_are_what_the_rule_gives_on_the_measured_profile():
    """profiles/transcript_rng_bench.txt ends with the toolbox's rule applied to its own rows; the library's defaults say the same, and the
    accessors set and get"""
    import re
    text = open(os.path.join(ROOT, "profiles", "transcript_rng_bench.txt")).read()
    rule = {k: (2**32 - 1 if v == "never" else int(v)) for k, v in re.findall(r"^rule: (\w+) +min_batch = (\w+)", text, re.M)}
    assert set(rule) == {"witness_rng", "challenge_scalars", "append_points"}
    for what, want in rule.items():
        get, set_ = getattr(T, "get_%s_min_batch" % what), getattr(T, "set_%s_min_batch" % what)
        assert get() == want, what
        set_(7)
        assert get() == 7
        set_(want)
    # the rule over the file's own verdicts: per call, the smallest N from which every row at that N and above says "device AHEAD"
    rows = re.findall(r"^(\w+) .*N = +(\d+) .*(device AHEAD|host AHEAD|within the spread)$", text, re.M)
    assert len(rows) == 4 * 6
    for what, want in rule.items():
        ahead = {}
        for name, n, verdict in rows:
            if name == what:
                ahead[int(n)] = ahead.get(int(n), True) and verdict == "device AHEAD"
        best = 2**32 - 1
        for n in sorted(ahead, reverse=True):
            if not ahead[n]:
                break
            best = n
        assert best == want, what


def test_lane_code_equals_host_merlin_under_sanitizers(tmp_path):
    """tests/host/transcript_rng_host_main.cpp + host/merlin.cpp, g++ -fsanitize=address,undefined, as a child process: 171 states x W x labels x
    counts through the lane code's witness RNG against Strobe128 / TranscriptRng, every state x label through get_challenge, every state x
    kind x label through the point appends against Transcript, on heap blocks of exactly each buffer's size."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "transcript_rng_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "transcript_rng_host_main.cpp"), os.path.join(ROOT, "zkp_amd", "csrc", "host", "merlin.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    cases = 3 * 171 * len(W)
    assert r.stdout.split("\n")[:-1] == ["rng_scalars %d 0" % (cases * len(SCALAR_COUNTS)), "rng_bytes %d 0" % (cases * len(BYTE_COUNTS)),
                                         "challenge_scalars %d 0" % (3 * 171), "append_points %d 0" % (3 * 171 * 3 * 2), "validate %d 0" % (3 * 171 * 3 * 2),
                                         "positions 166"]


def test_or_ballot_example_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "or_ballot_batch.py"), "64", "--host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert "ballots verified: 64 of 64" in lines and "m = 2 ballot: rejected" in lines and "swapped c_0 ballot: rejected" in lines
    cast = int(np.random.default_rng(64).integers(0, 2, size=64).sum())
    assert "tally: %d yes of 64 (cast: %d)" % (cast, cast) in lines

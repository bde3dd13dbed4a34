"""Hash to the group on the host backend (ctx == NULL): RFC 9496 section 4.3.4 FROM_UNIFORM_BYTES -- curve25519-dalek's
RistrettoPoint::from_uniform_bytes / hash_from_bytes::<Sha512> -- through zkp_from_uniform_bytes_batch, and the VRF example's
`hash_to_group` (reference tests/sig_and_vrf_example.rs:36-40) through zkp_hash_to_group_batch.  The host backend compiles the very
formulas of zkp_amd/csrc/ge25519.h the kernel runs; the independent checks are the RFC's published vectors and the oracle (C restatement
and Python model).  No GPU needed."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from zkp_amd import toolbox as T

P = 2**255 - 19

# RFC 9496 appendix A.3: SHA-512 of each label, then FROM_UNIFORM_BYTES, gives the encoding
RFC_A3 = [
    (b"Ristretto is traditionally a short shot of espresso coffee", "3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46"),
    (b"made with the normal amount of ground coffee but extracted with", "f26e5b6f7d362d2d2a94c5d0e7602cb4773c95a2e5c31a64f133189fa76ed61b"),
    (b"about half the amount of water in the same amount of time", "006ccd2a9e6867e6a2c5cea83d3302cc9de128dd2a9a57dd8ee7b9d7ffe02826"),
    (b"by using a finer grind.", "f8f0c87cf237953c5890aec3998169005dae3eca1fbb04548c635953c817f92a"),
    (b"This produces a concentrated shot of coffee per volume.", "ae81e7dedf20a497e10c304a765c1767a42d6e06029758d2d7e8ef7cc4c41179"),
    (b"Just pulling a normal shot short will produce a weaker shot", "e2705652ff9f5e44d3e841bf1c251cf7dddb77d140870d1ab2ed64f1a9ce8628"),
    (b"and is not a Ristretto as some believe.", "80bd07262511cdde4863f8a7434cef696750681cb9510eea557088f76d9e5065"),
]


def _half(x: int) -> bytes:
    return x.to_bytes(32, "little")


def _square_case(half: bytes) -> bool:
    """whether u v of the Elligator map of this 32-byte half is a square (RFC 9496 4.3.4: the was_square branch)"""
    t = (int.from_bytes(half, "little") & ((1 << 255) - 1)) % P
    r = M.SQRT_M1 * t * t % P
    u = (r + 1) * M.ONE_MINUS_D_SQ % P
    v = (-1 - r * M.D) * (r + M.D) % P
    return M.sqrt_ratio_m1(u, v)[0]


def edge_inputs() -> np.ndarray:
    """[k][64]: zero, all-ones, bit 255 set in either half, halves p, p + 1, 2^255 - 1 (not canonical), one half zero, halves of both
    Elligator branches"""
    rng = np.random.default_rng(9496)
    rnd = lambda: rng.bytes(32)                                          # noqa: E731
    sq = [h for h in (rnd() for _ in range(64)) if _square_case(h)][:2]
    nsq = [h for h in (rnd() for _ in range(64)) if not _square_case(h)][:2]
    assert len(sq) == 2 and len(nsq) == 2
    hi = lambda h: h[:31] + bytes([h[31] | 0x80])                        # noqa: E731
    rows = [bytes(64), b"\xff" * 64, hi(rnd()) + rnd(), rnd() + hi(rnd()), hi(rnd()) + hi(rnd()),
            _half(P) + _half(P), _half(P + 1) + _half(P + 1), _half(2**255 - 1) * 2, _half(P) + _half(2**255 - 1), _half(P - 1) + _half(1),
            bytes(32) + rnd(), rnd() + bytes(32), sq[0] + sq[1], nsq[0] + nsq[1], sq[0] + nsq[0], nsq[1] + sq[1], _half(P) + bytes(32)]
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 64).copy()


def oracle_map(rows) -> np.ndarray:
    return np.frombuffer(b"".join(C.from_uniform_bytes(bytes(r)) for r in rows), np.uint8).reshape(-1, 32)


def model_blob(t: M.Transcript) -> bytes:
    """the oracle model's merlin state in the 208-byte layout of zkp_toolbox.h: STROBE state, pos, pos_begin, cur_flags, padding"""
    s = t.strobe
    return bytes(s.state) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


@pytest.fixture(scope="module")
def oracle():
    C.build()


def test_rfc9496_a3_vectors_on_the_host(oracle):
    want = [bytes.fromhex(h) for _, h in RFC_A3]
    got = T.hash_from_bytes_sha512(None, [m for m, _ in RFC_A3])
    assert [bytes(g) for g in got] == want
    wide = np.frombuffer(b"".join(hashlib.sha512(m).digest() for m, _ in RFC_A3), np.uint8).reshape(-1, 64)
    assert [bytes(g) for g in T.from_uniform_bytes(None, wide, threads=1)] == want
    assert [bytes(g) for g in oracle_map(wide)] == want
    assert [M.ristretto_encode(M.ristretto_hash_from_bytes_sha512(m)) for m, _ in RFC_A3] == want


def test_edge_inputs_equal_the_oracle(oracle):
    rows = edge_inputs()
    got = T.from_uniform_bytes(None, rows)
    assert (got == oracle_map(rows)).all()
    for r, g in zip(rows, got):
        assert bytes(g) == M.ristretto_encode(M.ristretto_from_uniform_bytes(bytes(r)))
    # bit 255 is ignored and a half is read modulo p
    assert bytes(got[5]) == bytes(T.from_uniform_bytes(None, np.frombuffer(bytes(64), np.uint8).reshape(1, 64))[0])
    assert (T.from_uniform_bytes(None, np.frombuffer(_half(P + 1) * 2, np.uint8).reshape(1, 64)) ==
            T.from_uniform_bytes(None, np.frombuffer(_half(1) * 2, np.uint8).reshape(1, 64))).all()


def test_random_inputs_equal_the_oracle(oracle):
    rng = np.random.default_rng(4304)
    rows = rng.integers(0, 256, size=(2500, 64), dtype=np.uint8)
    got = T.from_uniform_bytes(None, rows, threads=4)
    assert (got == oracle_map(rows)).all()
    for i in range(0, len(rows), 97):
        assert bytes(got[i]) == M.ristretto_encode(M.ristretto_from_uniform_bytes(bytes(rows[i])))
    # every output is a valid canonical encoding, and the thread count does not change a byte
    assert (T.from_uniform_bytes(None, rows[:300], threads=1) == got[:300]).all()


def _model_transcripts(msgs):
    ts = []
    for i, m in enumerate(msgs):
        t = M.Transcript(b"VRF-function %d" % (i % 3))
        t.append_message(b"msg", m)
        ts.append(t)
    return ts


def _product_transcripts(msgs):
    ts = []
    for i, m in enumerate(msgs):
        t = T.Transcript(b"VRF-function %d" % (i % 3))
        t.append_message(b"msg", m)
        ts.append(t)
    return ts


@pytest.mark.parametrize("ragged", [False, True])
def test_hash_to_group_advances_transcripts_like_merlin(oracle, ragged):
    rng = np.random.default_rng(7 + ragged)
    n = 150
    msgs = [rng.bytes(int(rng.integers(0, 300)) if ragged else 40) for _ in range(n)]
    mts = _model_transcripts(msgs)
    want = [M.ristretto_encode(M.ristretto_from_uniform_bytes(t.challenge_bytes(b"output", 64))) for t in mts]
    # Transcript objects
    pts = _product_transcripts(msgs)
    got = T.hash_to_group(None, pts, threads=3)
    assert [bytes(g) for g in got] == want
    assert [t.state.tobytes() for t in pts] == [model_blob(t) for t in mts]
    # the state was advanced: a second squeeze agrees
    assert [t.challenge_bytes(b"again", 48) for t in pts] == [t.challenge_bytes(b"again", 48) for t in mts]
    # a [N][208] array, another label
    arr = np.stack([t.state for t in _product_transcripts(msgs)])
    mts = _model_transcripts(msgs)
    want = [M.ristretto_encode(M.ristretto_from_uniform_bytes(t.challenge_bytes(b"H", 64))) for t in mts]
    assert [bytes(g) for g in T.hash_to_group(T.HostEngine(), arr, label=b"H")] == want
    assert [r.tobytes() for r in arr] == [model_blob(t) for t in mts]


def test_argument_errors_and_empty_calls():
    lib = T.lib()
    out = np.zeros((4, 32), np.uint8)
    inp = np.zeros((4, 64), np.uint8)
    ts = np.stack([T.Transcript(b"x").state] * 4)
    before = ts.copy()
    assert lib.zkp_from_uniform_bytes_batch(None, ctypes.c_uint64(4), None, 0, T._p(out)) == T_BAD
    assert lib.zkp_from_uniform_bytes_batch(None, ctypes.c_uint64(4), T._p(inp), 0, None) == T_BAD
    assert lib.zkp_from_uniform_bytes_batch(None, ctypes.c_uint64(0), None, 0, None) == 0
    assert lib.zkp_hash_to_group_batch(None, ctypes.c_uint32(4), T._p(ts), None, 0, T._p(out)) == T_BAD
    assert lib.zkp_hash_to_group_batch(None, ctypes.c_uint32(4), None, b"output", 0, T._p(out)) == T_BAD
    assert lib.zkp_hash_to_group_batch(None, ctypes.c_uint32(4), T._p(ts), b"output", 0, None) == T_BAD
    assert lib.zkp_hash_to_group_batch(None, ctypes.c_uint32(0), None, b"output", 0, None) == 0
    assert (ts == before).all() and not out.any()
    assert T.from_uniform_bytes(None, np.zeros((0, 64), np.uint8)).shape == (0, 32)
    assert T.hash_to_group(None, []).shape == (0, 32)
    assert T.hash_from_bytes_sha512(None, []).shape == (0, 32)


T_BAD = -10          # ZKP_TB_BAD_STATEMENT: malformed statement descriptor / NULL argument

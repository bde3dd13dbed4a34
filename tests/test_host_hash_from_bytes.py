"""RistrettoPoint::hash_from_bytes::<Sha512> on the host backend (ctx == NULL): SHA-512 of zkp_amd/csrc/sha512.h -- the very text the
kernel k_sha512_csr compiles -- then the map, through zkp_hash_from_bytes_sha512_batch over CSR batches of messages.  The independent
checks are hashlib, the oracle's map and RFC 9496's vectors.  sha512.h's range clamp is checked on its own by a stand-alone driver built
with AddressSanitizer and UBSan.  No GPU needed."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cbind as C
from tests.test_host_hash_to_group import RFC_A3, oracle_map
from zkp_amd import toolbox as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA512_H = os.path.join(ROOT, "zkp_amd", "csrc", "sha512.h")
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
HEX_H = "90ca11cd6c6227cb0abc39e2710c444ae6617ea81898e716353f3410d9656605"      # examples/dleq_c_abi.c: hash_from_bytes::<Sha512>(B)
T_BAD = -10          # ZKP_TB_BAD_STATEMENT
PAD_EDGES = (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 241, 255, 256)


def sweep_batch():
    """One shared buffer holding every length 0..300, 1,000 and 65,536 at every start offset 0..15 (mod 16) as a CSR batch.  Filler
    messages between them set the start offsets; they are messages of the batch like any other.  -> (data, offsets, lengths of interest
    as (index, length, start))"""
    rng = np.random.default_rng(512)
    lengths = list(range(301)) + [1000, 65536]
    msgs, marks, pos = [], [], 0
    for start in range(16):
        for n in lengths:
            gap = (start - pos) % 16
            if gap:
                msgs.append(rng.bytes(gap))
                pos += gap
            marks.append((len(msgs), n, start))
            msgs.append(rng.bytes(n))
            pos += n
    data = np.frombuffer(b"".join(msgs), np.uint8).copy()
    offsets = np.zeros(len(msgs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs])
    return data, offsets, marks


def csr_messages(data, offsets):
    return [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(offsets) - 1)]


def want_points(messages) -> np.ndarray:
    """hashlib.sha512, then the oracle's ristretto_from_uniform_bytes"""
    wide = np.frombuffer(b"".join(hashlib.sha512(m).digest() for m in messages), np.uint8).reshape(-1, 64)
    return oracle_map(wide) if len(wide) else np.zeros((0, 32), np.uint8)


def random_batch(n, seed, max_len=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(0, 256, size=max(int(offsets[-1]), 1), dtype=np.uint8)
    return data, offsets


@pytest.fixture(scope="module")
def oracle():
    C.build()


def test_length_and_offset_sweep_equals_hashlib_and_the_oracle(oracle):
    data, offsets, marks = sweep_batch()
    got = T.hash_from_bytes_sha512_csr(None, data, offsets, threads=8)
    msgs = csr_messages(data, offsets)
    assert (got == want_points(msgs)).all()
    assert sorted({(n, s) for _, n, s in marks if n in PAD_EDGES and s in (0, 3)}) == sorted({(n, s) for n in PAD_EDGES for s in (0, 3)})
    # the same messages one by one, each at offset 0 of a buffer of its own
    for i, n, s in marks:
        if n in PAD_EDGES or n == 65536:
            assert bytes(T.hash_from_bytes_sha512(None, [msgs[i]])[0]) == bytes(got[i]), (n, s)


def test_rfc9496_vectors_and_the_c_example_generator(oracle):
    assert [bytes(g) for g in T.hash_from_bytes_sha512(None, [m for m, _ in RFC_A3])] == [bytes.fromhex(h) for _, h in RFC_A3]
    assert bytes(T.hash_from_bytes_sha512(None, [BASEPOINT])[0]).hex() == HEX_H
    assert C.from_uniform_bytes(hashlib.sha512(BASEPOINT).digest()).hex() == HEX_H


def test_rerouted_call_returns_what_the_python_route_returned(oracle):
    """hash_from_bytes_sha512 used to run hashlib per message and then from_uniform_bytes: same bytes through the C call, any thread count"""
    rng = np.random.default_rng(35)
    msgs = [rng.bytes(int(rng.integers(0, 400))) for _ in range(700)] + [b"", b"A VRF input, for instance"]
    old = T.from_uniform_bytes(None, np.frombuffer(b"".join(hashlib.sha512(m).digest() for m in msgs), np.uint8).reshape(-1, 64))
    for threads in (0, 1, 5):
        assert (T.hash_from_bytes_sha512(None, msgs, threads=threads) == old).all()
    assert (T.hash_from_bytes_sha512(T.HostEngine(), msgs[:9]) == old[:9]).all()
    data, offsets = random_batch(257, 36)
    assert (T.hash_from_bytes_sha512_csr(None, data, offsets) == want_points(csr_messages(data, offsets))).all()
    # offsets need not start at 0: a batch in the middle of a buffer
    assert (T.hash_from_bytes_sha512_csr(None, data, offsets[100:201]) == T.hash_from_bytes_sha512_csr(None, data, offsets)[100:200]).all()


def test_argument_errors_and_empty_calls():
    lib = T.lib()
    data = np.arange(64, dtype=np.uint8)
    out = np.zeros((3, 32), np.uint8)
    dec = np.array([0, 10, 5, 20], np.uint64)
    ok = np.array([0, 5, 10, 20], np.uint64)
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(3), T._p(data), T._p(dec), 0, T._p(out)) == T_BAD
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(3), None, T._p(ok), 0, T._p(out)) == T_BAD
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(3), T._p(data), None, 0, T._p(out)) == T_BAD
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(3), T._p(data), T._p(ok), 0, None) == T_BAD
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(0), None, None, 0, None) == 0
    assert not out.any()
    assert lib.zkp_hash_from_bytes_sha512_batch(None, ctypes.c_uint64(3), T._p(data), T._p(ok), 0, T._p(out)) == 0
    assert out.any()
    assert T.hash_from_bytes_sha512(None, []).shape == (0, 32)
    assert T.hash_from_bytes_sha512_csr(None, np.zeros(0, np.uint8), np.zeros(1, np.uint64)).shape == (0, 32)
    with pytest.raises(ValueError):
        T.hash_from_bytes_sha512_csr(None, data, dec)
    with pytest.raises(ValueError):
        T.hash_from_bytes_sha512_csr(None, data, np.array([0, 65], np.uint64))      # past the end of data


DRIVER = r"""
#include "sha512.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
// argv[1]: a file of cases "msgs_len lo hi"; the buffer is a heap block of exactly msgs_len bytes, byte i = (i * 131 + 7) mod 256.
// Prints, per case, the clamped lo and length, then the digest.
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "r");
  unsigned long long L, lo, hi;
  while (fscanf(f, "%llu %llu %llu", &L, &lo, &hi) == 3) {
    uint8_t* b = static_cast<uint8_t*>(malloc(L));
    for (unsigned long long i = 0; i < L; ++i) b[i] = (uint8_t)(i * 131 + 7);
    uint64_t clo = lo;
    const uint64_t len = zkp::sha512_clamp(clo, hi, L);
    uint64_t H[8];
    uint32_t w[16];
    zkp::sha512_range(H, b, L, lo, hi);
    zkp::sha512_digest_words(w, H);
    uint8_t d[64];
    memcpy(d, w, 64);
    printf("%llu %llu ", (unsigned long long)clo, (unsigned long long)len);
    for (int i = 0; i < 64; ++i) printf("%02x", d[i]);
    printf("\n");
    free(b);
  }
  fclose(f);
  return 0;
}
"""


def test_clamp_helper_under_sanitizers(tmp_path):
    """sha512_clamp and sha512_range of sha512.h alone, g++ -fsanitize=address,undefined: hi < lo, ranges past the end of a heap block
    that ends exactly at msgs_len, offsets near 2^64, and the padding edges at the very end of the buffer.  Each digest equals hashlib
    of the clamped range, and the sanitizers stay silent."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    src = tmp_path / "clamp_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "clamp_driver"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-Wno-unknown-pragmas", "-I", os.path.dirname(SHA512_H), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    top = 2**64 - 1
    cases = [(300, 20, 10), (300, 299, 0), (300, 0, 301), (300, 250, 1000), (300, 301, 400), (300, 400, 301), (300, top, top),
             (300, 5, top), (300, top, 5), (0, 0, 0), (0, 0, 10), (0, 7, 3), (1, 0, 1), (1, 0, 2), (1, 1, 1), (17, 3, 17), (17, 16, 99)]
    for n in (111, 112, 127, 128, 239, 240):
        for lead in (0, 1, 3, 5):                                    # the message ends exactly at msgs_len, starting at any byte offset
            cases.append((lead + n, lead, lead + n))
            cases.append((lead + n, lead, lead + n + 8))             # ... and a hi past the end
            cases.append((lead + n + 1, lead, lead + n))             # one byte of the buffer after it
    (tmp_path / "cases.txt").write_text("".join("%d %d %d\n" % c for c in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (L, lo, hi), line in zip(cases, lines):
        buf = bytes((i * 131 + 7) & 255 for i in range(L))
        clo = min(lo, L)
        chi = max(min(hi, L), clo)
        got_lo, got_len, digest = line.split()
        assert (int(got_lo), int(got_len)) == (clo, chi - clo), (L, lo, hi)
        assert digest == hashlib.sha512(buf[clo:chi]).hexdigest(), (L, lo, hi)

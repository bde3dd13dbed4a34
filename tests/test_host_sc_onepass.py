"""zkp_amd/csrc/sc25519.h, every function, on the host against Python integers.  The header is one text for g++ and hipcc: the one-pass
reduction mod l = 2^252 + delta (sc_reduce_wide, sc_reduce_384, sc_reduce_tail), the products on top of it (sc_mul, sc_muladd,
sc_mul_u128, sc_from_wide, sc_reduce) and the Montgomery product of the inversion chain, which skips the zero limbs of l.
tests/host/sc_onepass_host_main.cpp is built with g++ -fsanitize=address,undefined and runs as a child process with every operand in a
heap block of exactly its size.  No GPU needed.

Operands: the 256-bit edge catalogue of tests/scalar_edge_cases.py crossed with itself; l, 2 l and 2^256 - 1 as first operands; products
and sums that land on l - 1, l, 2 l - 1 and on both sides of every sign change of the last reduction step; the wide strings 0, l, 2^256,
2^512 - 1 and the largest multiple of l; 2,000 random records."""
import os
import random
import shutil
import subprocess

from tests import scalar_edge_cases as E
from tests.scalar_edge_cases import L, VALUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M256 = 2**256 - 1
DELTA = L - 2**252
R = 2**256
RINV = pow(R, -1, L)
Q512 = (2**512 - 1) // L * L                                   # the largest multiple of l below 2^512
WIDE_EDGES = [0, L, 2**256, 2**512 - 1, Q512, Q512 - 1, Q512 + 1, L << 256, 2**256 + L, 2**252, 2**504, (2**252 - 1) << 252]
FIRST = [L, 2 * L, M256]

(REDUCE, TO_MONT, MONT, MUL, MULADD, MUL_U128, ADD, NEG, FROM_WIDE, HALVE, HALVE_CANONICAL, INVERT, FOLD_SIGN, NOT_CANONICAL, COND_SUB_L,
 ADD_PATTERN, REDUCE_384, REDUCE_WIDE, SQMUL, MULADD_ALIAS_A, MUL_ALIAS_B, REDUCE_TAIL) = range(22)


def want(op, a, b, c):
    """the fields the program prints for one record, as integers"""
    if op == REDUCE:
        return [a % L]
    if op == TO_MONT:
        return [a * R % L]
    if op == MONT:
        return [a * b * RINV % L]
    if op in (MUL, MUL_ALIAS_B):
        return [a * b % L]
    if op in (MULADD, MULADD_ALIAS_A):
        return [(a * b + c) % L]
    if op == MUL_U128:
        return [a * (b % 2**128) % L]
    if op == ADD:
        return [(a + b) % L]
    if op == NEG:
        return [-a % L]
    if op in (FROM_WIDE, REDUCE_WIDE):
        return [(a + (b << 256)) % L]
    if op == HALVE:
        return [a * pow(2, -1, L) % L]
    if op == HALVE_CANONICAL:
        return [a * pow(2, -1, L) % L]
    if op == INVERT:
        return [pow(a % L, L - 2, L)]
    if op == FOLD_SIGN:
        return list(E.fold_sign(a))
    if op == NOT_CANONICAL:
        return [E.not_canonical(a)]
    if op == COND_SUB_L:
        return [a - L if a >= L else a]
    if op == ADD_PATTERN:
        e, top = E.add_pattern(a, b & 0xFFFFFFFF)
        return [E.from_words(e), top]
    if op == REDUCE_384:
        return [(a + ((b % 2**128) << 256)) % L]
    if op == SQMUL:
        y = a
        for _ in range(c & 7):
            y = y * y * RINV % L
        return [y * b * RINV % L]
    if op == REDUCE_TAIL:
        return [(a + ((c & 0xFFFFFFFF) << 256)) % L]
    raise AssertionError(op)


def records():
    rng = random.Random(20260101)
    recs = []
    n = len(VALUES)
    # the catalogue crossed with itself: the product alone, the product with a third catalogue value added, the Montgomery product
    for i, a in enumerate(VALUES):
        for j, b in enumerate(VALUES):
            c = VALUES[(i * 31 + j * 17) % n]
            recs += [(MUL, a, b, 0), (MULADD, a, b, c), (MONT, a, b % L, 0)]
    # l, 2 l and 2^256 - 1 as first operands (and, where the function takes any value there, as second and third)
    for f in FIRST:
        for v in VALUES:
            recs += [(MUL, f, v, 0), (MUL, v, f, 0), (MULADD, f, v, f), (MULADD, v, f, v), (MULADD_ALIAS_A, f, v, f), (MUL_ALIAS_B, f, v, 0),
                     (MONT, f, v % L, 0), (MUL_U128, f, v, 0), (REDUCE_384, f, v, 0), (FROM_WIDE, f, v, 0), (FROM_WIDE, v, f, 0)]
        recs += [(REDUCE, f, 0, 0), (TO_MONT, f, 0, 0), (HALVE, f, 0, 0), (INVERT, f, 0, 0)]
    # a * b + c (as an integer) on l - 2 .. l + 1 and 2 l - 2 .. 2 l + 1: the values a reduction that ended in conditional subtractions would
    # meet around its last one, and multiples of l further up
    for t in [L - 2, L - 1, L, L + 1, 2 * L - 2, 2 * L - 1, 2 * L, 2 * L + 1, 15 * L - 1, 15 * L, M256 * M256 // L * L, M256 * M256 // L * L - 1]:
        for a in (1, 2, 3, 2**128 - 1, 2**128 + 1, L - 1, M256):
            b = min(t // a, M256)
            c = t - a * b
            if 0 <= c <= M256:
                recs += [(MULADD, a, b, c), (MULADD, b, a, c), (MULADD_ALIAS_A, a, b, c)]
                if c == 0:
                    recs += [(MUL, a, b, 0), (MUL_ALIAS_B, b, a, 0)]
    # the last step (sc_reduce_tail) for every quotient q = v >> 252 it allows, at both ends of its range and on both sides of the sign
    # change of (v mod 2^252) - q delta
    for q in range(67):
        for vm in {0, 1, q * DELTA - 1, q * DELTA, q * DELTA + 1, 2**252 - 2, 2**252 - 1} - {-1}:
            v = (q << 252) + vm
            recs.append((REDUCE_TAIL, v & M256, 0, v >> 256))
            if q < 16:
                recs.append((REDUCE, v, 0, 0))
    # wide strings
    for w in WIDE_EDGES + [rng.getrandbits(512) for _ in range(100)] + [Q512 - k * L for k in range(1, 40)] + [k * L + d for k in (1, 2**130, 2**259) for d in (-1, 0, 1)]:
        recs += [(FROM_WIDE, w & M256, w >> 256, 0), (REDUCE_WIDE, w & M256, w >> 256, 0)]
    for w in [0, L, 2**256, 2**384 - 1, (2**384 - 1) // L * L, (2**384 - 1) // L * L - 1, 2**252, (2**132 - 1) << 252, 2**383]:
        recs.append((REDUCE_384, w & M256, w >> 256, 0))
    # the one-operand functions and those with a precondition, over the catalogue
    for i, v in enumerate(VALUES):
        w = VALUES[(i + 1) % n]
        recs += [(REDUCE, v, 0, 0), (TO_MONT, v, 0, 0), (HALVE, v, 0, 0), (INVERT, v, 0, 0), (FOLD_SIGN, v, 0, 0), (NOT_CANONICAL, v, 0, 0),
                 (ADD, v % L, w % L, 0), (ADD, v % L, L - 1, 0), (NEG, v % L, 0, 0), (HALVE_CANONICAL, v % L, 0, 0), (COND_SUB_L, v % (2 * L), 0, 0),
                 (MUL_U128, v, w, 0), (MUL_U128, v, 2**128 - 1, 0), (REDUCE_384, v, 2**128 - 1, 0), (SQMUL, v % L, w % L, i)]
        recs += [(ADD_PATTERN, v, p, 0) for p in E.PROBE_PATTERNS]
    recs += [(COND_SUB_L, v, 0, 0) for v in (0, L - 1, L, L + 1, 2 * L - 1)]
    # 2,000 random records, every function in turn
    for k in range(2000):
        op = k % 22
        a, b, c = (rng.getrandbits(256) for _ in range(3))
        if op == MONT:
            b %= L
        elif op in (ADD, SQMUL):
            a, b = a % L, b % L
        elif op in (NEG, HALVE_CANONICAL):
            a %= L
        elif op == COND_SUB_L:
            a %= 2 * L
        elif op == REDUCE_TAIL:
            v = rng.randrange(67 << 252)
            a, c = v & M256, v >> 256
        recs.append((op, a, b, c))
    return recs


def test_the_record_list_holds_what_it_promises():
    recs = records()
    n = len(VALUES)
    assert sum(1 for r in recs if r[0] == MUL) >= n * n and sum(1 for r in recs if r[0] == MULADD) >= n * n
    assert {r[0] for r in recs} == set(range(22))
    for f in FIRST:
        assert any(r[0] == MULADD and r[1] == f for r in recs) and any(r[0] == MONT and r[1] == f for r in recs)
    sums = {r[1] * r[2] + r[3] for r in recs if r[0] == MULADD}
    assert {L - 1, L, 2 * L - 1, 2 * L} <= sums
    wides = {r[1] + (r[2] << 256) for r in recs if r[0] == FROM_WIDE}
    assert {0, L, 2**256, 2**512 - 1, Q512} <= wides
    tails = {(r[1] + (r[3] << 256)) >> 252 for r in recs if r[0] == REDUCE_TAIL}
    assert set(range(67)) <= tails and max(tails) == 66


def test_every_function_of_the_scalar_header_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (it builds the host library too)"
    exe = tmp_path / "sc_onepass_host_main"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "host", "sc_onepass_host_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    recs = records()
    h = lambda v: v.to_bytes(32, "little").hex()
    (tmp_path / "records.txt").write_text("".join("%d %s %s %s\n" % (op, h(a), h(b), h(c)) for op, a, b, c in recs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(tmp_path / "records.txt")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(recs)
    bad = []
    for rec, line in zip(recs, lines):
        got = [int.from_bytes(bytes.fromhex(x), "little") for x in line.split()]
        if got != want(*rec):
            bad.append((rec[0], [hex(x) for x in rec[1:]], [hex(x) for x in got], [hex(x) for x in want(*rec)]))
    assert not bad, (len(bad), bad[:5])


def test_host_library_and_header_agree_on_muladd_and_from_wide():
    """the toolbox's host route (libzkp_toolbox.so: the same header at -O3) gives what the integers give, for operands that are not reduced"""
    import numpy as np

    from zkp_amd import toolbox as T
    rows = lambda vals, width=32: np.frombuffer(b"".join(int(v).to_bytes(width, "little") for v in vals), np.uint8).reshape(-1, width).copy()
    ints = lambda arr: [int.from_bytes(bytes(x), "little") for x in arr]
    a, b, c = VALUES, VALUES[::-1], VALUES[7:] + VALUES[:7]
    assert ints(T.scalar_muladd(None, rows(a), rows(b), rows(c))) == [(x * y + z) % L for x, y, z in zip(a, b, c)]
    wide = WIDE_EDGES + [x | (y << 256) for x, y in zip(a, b)]
    assert ints(T.scalar_from_wide(None, rows(wide, 64))) == [w % L for w in wide]

"""(helper module of tests/test_host_dlog_point.py and tests/test_gpu_dlog_point.py)
Operands of the bounded discrete logarithm to a base of the caller's, unsigned and signed, and what the call must return for them.

Bases: B itself, G7 = 7 B and H, the first of point_mul_cases.hashed_points().  Found rows are encode(k G) from oracle.cbind.msm_many with the base
row G and the scalar k mod l, for integers k this module chose: the expected output is k itself.  The k values are those of
dlog_cases.k_values (table, chunk, slice and range edges).  A signed range [-2^(bits - 1), 2^(bits - 1)) is searched as k' = k + 2^(bits - 1) in
[0, 2^bits), so in signed mode those values are used twice -- as k where they are below 2^(bits - 1), and as k' -- and joined by
-2^(bits - 1) and 2^(bits - 1) - 1 (found), 2^(bits - 1) and -2^(bits - 1) - 1 (not found), 0, +-1, +-(m - 1), +-m, +-chunk m, and the values on both
sides of every slice edge around the slice that starts at k = 0.

Spoilers between found rows: the encodings RFC 9496 appendix A.3 rejects, rows out of range, hashed points, and MULTIPLES OF ANOTHER BASE:
5 B and 15 B have no logarithm to H; 15 B has none to G7 while 14 B has logarithm 2 -- the table really is G's.  Nothing here calls the code
under test."""
import functools

import numpy as np

from oracle import cbind as C
from tests import dlog_cases as DC
from tests import point_mul_cases as PC
from tests.scalar_edge_cases import L

FOUND, INVALID, NOT_FOUND = DC.FOUND, DC.INVALID, DC.NOT_FOUND
BASES = ("B", "G7", "H")


@functools.lru_cache(maxsize=None)
def base(name) -> bytes:
    """the encoding of the base"""
    if name == "B":
        return PC.BASEPOINT
    if name == "G7":
        return bytes(DC.encode_multiples([7])[0])
    assert name == "H"
    return PC.hashed_points()[0]


@functools.lru_cache(maxsize=None)
def _encode(name, ks):
    C.build()
    n = len(ks)
    out, st = C.msm_many(np.arange(n + 1, dtype=np.uint32), PC.rows([k % L for k in ks]), np.zeros(n, np.uint32), PC.enc_rows([base(name)]), 0)
    assert not st.any()
    return out


def encode_multiples(name, ks) -> np.ndarray:
    """encode(k G) for integers k of either sign: uint8 [n][32]"""
    return _encode(name, tuple(int(k) for k in ks)).copy()


def other_bases(n) -> list:
    """n distinct valid bases that are none of BASES: (100 + i) B"""
    return [bytes(r) for r in DC.encode_multiples([100 + i for i in range(n)])]


def without_logarithm(name, signed):
    """valid encodings with no logarithm to the base in any range the call accepts"""
    rows = list(PC.hashed_points())[1:]
    if name == "B":
        rows.append(PC.hashed_points()[0])
    if name == "H":
        rows += [bytes(r) for r in DC.encode_multiples([5, 15])]
    if name == "G7":
        rows += [bytes(r) for r in DC.encode_multiples([15, 8])]
    if not signed:
        rows.append(bytes(encode_multiples(name, [L - 1])[0]))       # (-G: logarithm -1 in a signed range)
    return rows


def k_values(baby_bits, bits, chunk, slice_chunks=None, signed=False):
    """the integers k of the module's text for one (baby_bits, bits): (in range, out of range)"""
    inside, outside = DC.k_values(baby_bits, bits, chunk, slice_chunks)
    if not signed:
        return inside, outside
    m, half = 1 << baby_bits, 1 << (bits - 1)
    cand = list(inside) + [k - half for k in inside]                 # as k, and as k'
    cand += [-half, half - 1, half, -half - 1, 0, 1, -1, m - 1, 1 - m, m, -m, chunk * m, -chunk * m]
    if slice_chunks:
        s = slice_chunks * chunk * m
        for edge in (-2 * s, -s, 0, s, 2 * s):
            cand += [edge - 1, edge, edge + 1]
    cand += outside
    ins, outs, seen = [], [], set()
    for k in cand:
        if k in seen:
            continue
        seen.add(k)
        (ins if -half <= k < half else outs).append(k)
    return ins, sorted(outs)


@functools.lru_cache(maxsize=None)
def operands(name, baby_bits, bits, chunk, slice_chunks=None, signed=False):
    """(points [n][32], k [n] (int64 when signed, else uint64), status uint8 [n]): found rows with invalid, out-of-range and logarithm-free
    rows between them"""
    inside, outside = k_values(baby_bits, bits, chunk, slice_chunks, signed)
    spoil = [(bytes(r), INVALID) for r in PC.enc_rows(PC.invalid_points())]
    spoil += [(bytes(r), NOT_FOUND) for r in encode_multiples(name, outside)]
    spoil += [(p, NOT_FOUND) for p in without_logarithm(name, signed)]
    found = [bytes(r) for r in encode_multiples(name, inside)]
    if name == "G7" and (2 in inside):
        found.append(bytes(DC.encode_multiples([14])[0]))              # 14 B = 2 G7, from the table of B
        inside = inside + [2]
    pts, ks, st = [], [], []
    for i in range(max(len(inside), len(spoil))):
        pts.append(found[i % len(inside)]); ks.append(inside[i % len(inside)]); st.append(FOUND)
        if i < len(spoil):
            pts.append(spoil[i][0]); ks.append(0); st.append(spoil[i][1])
    pts.append(found[0]); ks.append(inside[0]); st.append(FOUND)          # (the last row is a found one as well)
    return PC.enc_rows(pts), np.array(ks, np.int64 if signed else np.uint64), np.array(st, np.uint8)


def tiled(name, baby_bits, bits, chunk, n, signed=False):
    """the first n rows of operands(...) repeated as often as needed"""
    p, k, s = operands(name, baby_bits, bits, chunk, None, signed)
    return PC.tiled(p, n), PC.tiled(k, n), PC.tiled(s, n)


def slice_order(n_slices, signed):
    """what zkp_dlog_slice_order must return for i = 0 .. n_slices - 1, from its description: unsigned the identity; signed the slice
    n_slices // 2 first, then alternately below and above it until both ends are reached"""
    if not signed:
        return list(range(n_slices))
    z = n_slices // 2
    out, d = [z], 1
    while len(out) < n_slices:
        if z - d >= 0:
            out.append(z - d)
        if z + d < n_slices:
            out.append(z + d)
        d += 1
    return out

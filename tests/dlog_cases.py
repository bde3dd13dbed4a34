"""(helper module of tests/test_host_dlog.py and tests/test_gpu_dlog.py)
Operands of the bounded discrete logarithm to the basepoint, and what the call must return for them.

Found rows are encode(k B) from oracle.cbind.msm_many for integers k this module chose: the expected output is k itself.  Rows without a
logarithm in range are outputs of the oracle's hash-to-group map and (l - 1) B; rows that do not decode are the encodings RFC 9496 appendix A.3
rejects (tests/point_mul_cases.py).  Invalid and not-found rows sit BETWEEN found ones, so that damage to a neighbour shows.

With m = 2^baby_bits, G = the giant steps of one work item (chunk) and S = the chunks of a point that one launch covers (slice), both read from the
product by the caller, the k values cover: 0, 1, m - 1, m, m + 1, 2m, 3m (multiples of m are the zero case of the shared inversion: the doubled
candidate is the identity), the chunk edges G m - 1, G m, G m + 1, the slice edges S G m - 1, S G m, S G m + 1, 2^bits - 1 (found) and 2^bits,
2^bits + 1 (not found); with bits <= baby_bits, baby indices at and above 2^bits (not found although their rows are in the table).  Nothing here calls
the code under test."""
import functools

import numpy as np

from oracle import cbind as C
from tests import point_mul_cases as PC
from tests.scalar_edge_cases import L

FOUND, INVALID, NOT_FOUND = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _encode(ks):
    C.build()
    n = len(ks)
    out, st = C.msm_many(np.arange(n + 1, dtype=np.uint32), PC.rows([k % L for k in ks]), np.zeros(n, np.uint32), PC.BASEPOINT_ROW, 0)
    assert not st.any()
    return out


def encode_multiples(ks) -> np.ndarray:
    """encode(k B) for integers k: uint8 [n][32]"""
    return _encode(tuple(int(k) for k in ks)).copy()


def without_logarithm():
    """valid encodings with no logarithm in any range the call accepts: hashed points and (l - 1) B"""
    return list(PC.hashed_points()) + [bytes(encode_multiples([L - 1])[0])]


def k_values(baby_bits, bits, chunk, slice_chunks=None):
    """the integers k of the module's text for one (baby_bits, bits): (in range, out of range)"""
    m = 1 << baby_bits
    edges = [0, 1, m - 1, m, m + 1, 2 * m, 3 * m, chunk * m - 1, chunk * m, chunk * m + 1, 2 * chunk * m, (1 << bits) - 1, (1 << bits) // 2, 5 % (1 << bits)]
    if slice_chunks:
        s = slice_chunks * chunk * m
        edges += [s - 1, s, s + 1, 2 * s, 2 * s + m - 1]
    rng = np.random.default_rng(1000 * baby_bits + bits)
    edges += [int(x) for x in rng.integers(0, 1 << bits, size=6)]
    inside, seen = [], set()
    for k in edges:
        if 0 <= k < (1 << bits) and k not in seen:
            seen.add(k)
            inside.append(k)
    outside = [1 << bits, (1 << bits) + 1]
    if bits < baby_bits:
        outside += [m - 1, m, (1 << bits) + 2]                       # m - 1: a baby row, but not below 2^bits
    if bits <= 47:
        outside.append((1 << bits) + (1 << baby_bits) * chunk + 3)
    return inside, sorted(set(outside))


@functools.lru_cache(maxsize=None)
def operands(baby_bits, bits, chunk, slice_chunks=None):
    """(points [n][32], k uint64 [n], status uint8 [n]): found rows with invalid, out-of-range and logarithm-free rows between them"""
    inside, outside = k_values(baby_bits, bits, chunk, slice_chunks)
    spoil = [(bytes(r), INVALID) for r in PC.enc_rows(PC.invalid_points())]
    spoil += [(bytes(r), NOT_FOUND) for r in encode_multiples(outside)]
    spoil += [(p, NOT_FOUND) for p in without_logarithm()]
    found = encode_multiples(inside)
    pts, ks, st = [], [], []
    for i in range(max(len(inside), len(spoil))):
        k = inside[i % len(inside)]
        pts.append(bytes(found[i % len(inside)])); ks.append(k); st.append(FOUND)
        if i < len(spoil):
            pts.append(spoil[i][0]); ks.append(0); st.append(spoil[i][1])
    pts.append(bytes(found[0])); ks.append(inside[0]); st.append(FOUND)          # (the last row is a found one as well)
    return PC.enc_rows(pts), np.array(ks, np.uint64), np.array(st, np.uint8)


def tiled(baby_bits, bits, chunk, n, slice_chunks=None):
    """the first n rows of operands(...) repeated as often as needed"""
    p, k, s = operands(baby_bits, bits, chunk, slice_chunks)
    return PC.tiled(p, n), PC.tiled(k, n), PC.tiled(s, n)


def small_mixed(n, bits, seed=3):
    """n points with logarithms drawn from [0, 2^bits), most of them small: (points, k)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << bits, size=n)
    k[rng.random(n) < 0.7] %= 97
    uniq, inv = np.unique(k, return_inverse=True)
    return encode_multiples(uniq)[inv], k.astype(np.uint64)

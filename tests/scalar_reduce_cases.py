"""(helper module of tests/test_host_scalar_reduce.py and tests/test_gpu_scalar_reduce.py)
Jobs for the segmented scalar sums, products and dot products (zkp_sc_reduce, zkp_scalar_reduce_batch) and their expected values.

A job is (op, off, a, aidx, b, bidx) with a and b as lists of Python integers below 2^256 (any 32 bytes are an operand).  Expected values are
Python integers mod l, computed here and nowhere else; nothing in this module calls the code under test.  Lengths are given in units of the
fold's group size G, which the caller passes in (the GPU tests read it from zkp_sc_reduce_group(), the host tests use the same lengths)."""
import numpy as np

from tests.scalar_edge_cases import L, VALUES, random_256

SUM, PRODUCT, DOT = 0, 1, 2
OPS = (SUM, PRODUCT, DOT)
EDGES = list(dict.fromkeys([0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 256 - 1] + VALUES))


def rows(vals):
    """integers below 2^256 -> uint8 [n][32], little endian"""
    if len(vals) == 0:
        return np.zeros((0, 32), np.uint8)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


def ints(arr):
    return [int.from_bytes(bytes(r), "little") for r in np.asarray(arr, np.uint8).reshape(-1, 32)]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def expected(op, off, a, aidx=None, b=None, bidx=None):
    """the integers mod l of every output"""
    out = []
    for i in range(len(off) - 1):
        acc = 1 if op == PRODUCT else 0
        for t in range(int(off[i]), int(off[i + 1])):
            x = a[t if aidx is None else int(aidx[t])]
            if op == SUM:
                acc = (acc + x) % L
            elif op == PRODUCT:
                acc = acc * x % L
            else:
                acc = (acc + x * b[t if bidx is None else int(bidx[t])]) % L
        out.append(acc)
    return out


def operands(op, t, seed):
    """(a, b): t random 256-bit integers each (b = None unless DOT); products stay non-zero so that a wrong factor shows"""
    a = random_256(seed, t)
    if op == PRODUCT:
        a = [v if v % L else 3 for v in a]
    return a, (random_256(seed + 1000, t) if op == DOT else None)


def job(op, lens, seed=1):
    """(op, off, a, None, b, None): one row per term"""
    off = offsets(lens)
    a, b = operands(op, int(off[-1]), seed)
    return op, off, a, None, b, None


def single_lengths(G):
    return [0, 1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 7]


def ragged_lengths(G=256):
    """about 900 terms: leading, inner and trailing empty segments, many segments inside one group, one 600-term segment that five threads cut (and
    that spans three groups of 256)"""
    return [0, 0, 1, 2, 3, 0, 5, 1, 1, 7, 40, 0, 0, 2, 600, 1, 90, 0, 33, 64, 2, 1, 0, 47, 0, 0]


def positions(n, G):
    """first, last and group-edge positions of a segment of n terms that starts at a group edge"""
    return sorted({p for p in (0, 1, n - 1, G - 1, G, G + 1, 2 * G - 1, 2 * G) if 0 <= p < n})


def edge_rotation(op, G, shift):
    """one segment of 2 G + 3 terms between two short ones, the first at a group edge: the catalogue's values at the first, last and group-edge
    positions of the long segment, rotated by `shift`; a zero is a legitimate factor here"""
    lens = [G, 2 * G + 3, 5]
    off = offsets(lens)
    a, b = operands(op, int(off[-1]), 50 + shift)
    for k, p in enumerate(positions(lens[1], G)):
        a[G + p] = EDGES[(k + shift) % len(EDGES)]
        if b is not None:
            b[G + p] = EDGES[(k + 2 * shift + 3) % len(EDGES)]
    return op, off, a, None, b, None


def product_with_zero_at(G, p):
    """segments [G, 2 G + 3, 5] of non-zero factors, a zero at position p of the long one: that product is 0, its neighbours are not"""
    op, off, a, _, _, _ = job(PRODUCT, [G, 2 * G + 3, 5], seed=70 + p)
    a[G + p] = [0, L, 2 * L][p % 3]
    return op, off, a, None, None, None


def gathers(op, G):
    """jobs with repeated indices: all indices 0, a matrix column, and j^i for i = 0 .. G + 1 (PRODUCT) / i * x_j (SUM) / sum x_j y_j i times (DOT)"""
    jobs = []
    a, b = operands(op, 9, 90)
    lens = [0, 1, G + 2, 3]
    off = offsets(lens)
    t = int(off[-1])
    jobs.append((op, off, a, np.zeros(t, np.uint32), b, None if b is None else np.zeros(t, np.uint32)))
    # a matrix [r][c] stored row-major, output j folds column j (DOT: against the vector b gathered by row number)
    r, c = G + 3, 5
    m, v = operands(op, r * c, 91)
    off = offsets([r] * c)
    aidx = np.array([i * c + j for j in range(c) for i in range(r)], np.uint32)
    vec = None if v is None else v[:r]
    jobs.append((op, off, m, aidx, vec, None if v is None else np.array([i for j in range(c) for i in range(r)], np.uint32)))
    # powers: output i references row j i times, i = 0 .. G + 1
    base, other = operands(op, 3, 92)
    j = 2
    lens = list(range(G + 2))
    off = offsets(lens)
    t = int(off[-1])
    jobs.append((op, off, base, np.full(t, j, np.uint32), other, None if other is None else np.full(t, 1, np.uint32)))
    return jobs


def with_arange(jb):
    """the same job with the index lists written out"""
    op, off, a, aidx, b, bidx = jb
    t = int(off[-1])
    return op, off, a, np.arange(t, dtype=np.uint32) if aidx is None else aidx, b, (np.arange(t, dtype=np.uint32) if bidx is None and b is not None else bidx)


def level_edges(levels_fn, limit=1 << 22):
    """[(level count, smallest T with it)] for every level count a T <= limit has, by bisection on the library's zkp_sc_reduce_levels"""
    out = [(levels_fn(1), 1)]
    top = levels_fn(limit)
    while out[-1][0] < top:
        want = out[-1][0] + 1
        lo, hi = out[-1][1], limit                 # levels(lo) < want <= levels(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if levels_fn(mid) >= want:
                hi = mid
            else:
                lo = mid
        out.append((levels_fn(hi), hi))
    return out

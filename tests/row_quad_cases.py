"""Operands and expectations for the probes of the two layers on top of the field core (tests/test_rowfe_model.py, tests/test_host_fe_core.py,
tests/test_gpu_row_quad_probe.py):

  * zkp_amd/csrc/rowfe.h, one limb per lane (tools/microbench/row_probe.hip): full 64-lane register images, a row per coordinate.  Every row is
    chosen on its own from the class maximum, zero, one limb at its maximum, random limbs of the class, non-canonical forms of small values
    and real curve points.  The admission rule is the model (tools/model/rowfe_model.py): a record reaches the device only if the model runs it
    without Overflow, and the expected bytes are the model's images, idle lanes included.
  * zkp_amd/csrc/quad.h, a coordinate per lane of a quad (tools/microbench/quad_probe.hip): 2 x 4 x 9 raw limbs of the tight class; the
    expectation is the host build of fe25519.h making quad.h's calls lane by lane (tests/host/fe_core_host_lib.cpp: t_quad_probe), run in a
    child process because its bound-tracked build aborts on a violation."""
import ctypes
import functools
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools", "model")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import rowfe_model as R  # noqa: E402
from tests import fe_core_cases as K  # noqa: E402

P = K.P
# ---------------------------------------------------------------------------------------------------------------- row probe: file format
OP_MUL_AB, OP_MUL_AA, OP_CARRY, OP_POINT, OP_SQN = 1, 2, 4, 8, 16
OP_ALL = 31
ROW_OPS = ["row_mul(a,b)", "row_mul(a,a)", "row_carry(a)", "row_double(a)", "row_add_cached(a,b)", "11 x row_double + row_add_cached", "row_sqn(a,5)",
           "row_bcast01.a", "row_bcast01.b", "row_bcast23.a", "row_bcast23.b", "row_bcast_all.r0", "row_bcast_all.r1", "row_bcast_all.r2", "row_bcast_all.r3"]
ROW_MAX_W = 37
# the class pairs row_mul's callers use: (X + Y)^2, G x H of a doubling, (Y1 - X1) x cached, E x F after a carry, and the widest the model admits
ROW_MUL_PAIRS = [("sum", "sum"), ("diff", "sum"), ("diff", "tight"), ("tight", "diff"), ("extreme", "tight")]
PER_PAIR = 96
# (W, C): W windows of C doublings and one cached addition below the top window -- pip_run<C> runs k_pip_combine with W = W1 - 1 = ceil(256 / C) for
# C = 7, 10, 11, 16 (259, 260, 264, 256 doublings); (23, 11) is the 253 doublings of a canonical scalar's 23 full windows (pick_c's comment)
HORNER_SHAPES = [(37, 7), (26, 10), (24, 11), (16, 16), (23, 11)]

NONCANONICAL = {name: [(v >> (29 * k)) & ((1 << 29) - 1) for k in range(8)] + [v >> 232] for name, v in
                (("p", P), ("p+1", P + 1), ("p-1", P - 1), ("2^255-1", 2 ** 255 - 1), ("0", 0))}
ZERO_AS_P = NONCANONICAL["p"]                                          # == 0 with no limb zero


def limbs(v):
    return R.limbs_of(v % P)


def image(rows, rng=None):
    """4 x 9 limbs -> 64 lanes; the idle lanes 9 .. 15 of every row are zero, or garbage where rng is given"""
    out = [rng.randrange(2 ** 32) if rng else 0 for _ in range(64)]
    for r in range(4):
        out[16 * r:16 * r + 9] = rows[r]
    return out


def row_values(img):
    return [K.value(img[16 * r:16 * r + 9]) for r in range(4)]


def cached_of(q):
    return [(q[1] - q[0]) % P, (q[1] + q[0]) % P, 2 * q[2] % P, R.D2 * q[3] % P]


def add_cached_values(p, c):
    """the addition formula on raw row values: p = (X1, Y1, Z1, T1), c = (Y2 - X2, Y2 + X2, 2 Z2, 2 d T2)"""
    A, B, D, C = (p[1] - p[0]) * c[0] % P, (p[1] + p[0]) * c[1] % P, p[2] * c[2] % P, p[3] * c[3] % P
    E, H, F, G = (B - A) % P, (B + A) % P, (D - C) % P, (D + C) % P
    return [E * F % P, G * H % P, F * G % P, E * H % P]


IDENTITY = (0, 1, 1, 0)
IDENTITY_AS_P = [ZERO_AS_P, NONCANONICAL["p+1"], NONCANONICAL["p+1"], ZERO_AS_P]      # the same point, no coordinate canonical


def neg_point(q):
    return (-q[0] % P, q[1], q[2], -q[3] % P)


def point_pairs(rng, count):
    """(P, Q) with the identity on either side, P = Q, P = -Q, then random points (random Z each)"""
    a, b, c, d = (R.random_point(rng) for _ in range(4))
    pairs = [(IDENTITY, IDENTITY), (a, IDENTITY), (IDENTITY, b), (c, c), (d, neg_point(d))]
    while len(pairs) < count:
        pairs.append((R.random_point(rng), R.random_point(rng)))
    return pairs


def spread(pools, i, step):
    """row r of record i: entry i + r * step of the row's own pool, so the rows of one record mix edge and random operands"""
    return [pools[r][(i + r * step) % len(pools[r])] for r in range(4)]


EDGE_PAIRS = 7


def edge_pairs(ca, cb):
    """EDGE_PAIRS records (a rows, b rows) with BOTH operands of a row at an edge: maximum x maximum in every row (the largest columns the pair can
    make -- K.operands pairs a maximum with random limbs only), then a maximum against every single-limb maximum, from either side"""
    ma, mb = K.CLASSES[ca], K.CLASSES[cb]
    one = lambda m, j: [m[k] if k == j % 9 else 0 for k in range(9)]
    out = [([ma] * 4, [mb] * 4)]
    for e in range(3):
        out.append(([ma] * 4, [one(mb, 4 * e + r) for r in range(4)]))
    for e in range(3):
        out.append(([one(ma, 4 * e + r) for r in range(4)], [mb] * 4))
    return out


# ---------------------------------------------------------------------------------------------------------------- row probe: records
def row_candidates(seed=20251017):
    """main records as dicts kind / mask / a / b, before admission.  The kinds starting with "refused" are the pairs the model must refuse."""
    rng = random.Random(seed)
    recs = []

    def put(kind, mask, a_rows, b_rows, a_img=None, b_img=None):
        recs.append({"kind": kind, "mask": mask, "a": a_img or image(a_rows), "b": b_img or image(b_rows, rng)})

    for ca, cb in ROW_MUL_PAIRS:
        pa = [K.operands(rng, ca, PER_PAIR) for _ in range(4)]
        pb = [list(reversed(K.operands(rng, cb, PER_PAIR))) for _ in range(4)]
        mask = OP_MUL_AB | OP_CARRY | (OP_MUL_AA | OP_SQN if ca in K.SQ_CLASSES else 0)
        for i in range(PER_PAIR):
            put("mul %s x %s" % (ca, cb), mask, spread(pa, i, 24), spread(pb, i, 24))
        for a_rows, b_rows in edge_pairs(ca, cb):
            put("mul %s x %s" % (ca, cb), mask, a_rows, b_rows)
    # the tight class through every operation, point formulas included (polynomial identities: the rows need not be a curve point)
    pa = [K.operands(rng, "tight", PER_PAIR) for _ in range(4)]
    pb = [list(reversed(K.operands(rng, "tight", PER_PAIR))) for _ in range(4)]
    for i in range(PER_PAIR):
        put("tight x tight", OP_ALL, spread(pa, i, 24), spread(pb, i, 24))
    for a_rows, b_rows in edge_pairs("tight", "tight"):
        put("tight x tight", OP_ALL, a_rows, b_rows)
    nc = list(NONCANONICAL.values())
    for i in range(5):
        for j in range(5):
            put("non-canonical", OP_ALL, [nc[(i + r) % 5] for r in range(4)], [nc[(j + 2 * r) % 5] for r in range(4)])
    for p, q in point_pairs(rng, 48):
        put("points", OP_ALL, [limbs(v) for v in p], [limbs(v) for v in cached_of(q)])
    a = R.random_point(rng)                                            # the identity written with non-canonical zeros and ones, on either side
    put("points", OP_ALL, IDENTITY_AS_P, [limbs(v) for v in cached_of(a)])
    put("points", OP_ALL, [limbs(v) for v in a], [NONCANONICAL["p+1"], NONCANONICAL["p+1"], limbs(2), ZERO_AS_P])
    edge = K.operands(rng, "tight", 11) + nc
    for i, (p, q) in enumerate(point_pairs(rng, 16)):                  # a point with some rows replaced by edge operands
        a_rows, b_rows = [limbs(v) for v in p], [limbs(v) for v in cached_of(q)]
        for r in range(4):
            if (i >> r) & 1:
                a_rows[r] = edge[(i + 3 * r) % 16]
            else:
                b_rows[r] = edge[(5 * i + r) % 16]
        put("points with edge rows", OP_ALL, a_rows, b_rows)
    # row_carry: any 32-bit lanes
    full = 2 ** 32 - 1
    cpool = [[full] * 9, [0] * 8 + [full], [full] * 8 + [0]] + [[full if k == j else 0 for k in range(9)] for j in range(9)]
    cpool += [[full if k == j else rng.randrange(2 ** 32) for k in range(9)] for j in range(9)]
    while len(cpool) < 64:
        cpool.append([rng.randrange(2 ** 32) for _ in range(9)])
    for i in range(64):
        put("carry 32-bit lanes", OP_CARRY, spread([cpool] * 4, i, 16), spread([cpool] * 4, i, 5))
    # the lane index in every lane: the moves between rows alone (no arithmetic reads this record)
    put("lane index", 0, None, None, a_img=list(range(64)), b_img=list(range(63, -1, -1)))
    # what the model must refuse: a difference times a difference, and 2^32 - 1 in every limb
    diff = [K.CLASSES["diff"]] * 4
    put("refused diff x diff", OP_MUL_AB, diff, diff)
    put("refused 2^32-1 limbs", OP_MUL_AB, [[full] * 9] * 4, [K.TIGHT] * 4)
    return recs


def model_images(rec):
    """the ROW_OPS images of a main record through the model (zeros where the mask leaves an operation out); raises R.Overflow"""
    a, b, mask = rec["a"], rec["b"], rec["mask"]
    out = [[0] * 64 for _ in ROW_OPS]
    if mask & OP_MUL_AB:
        out[0] = R.row_mul(a, b)
    if mask & OP_MUL_AA:
        out[1] = R.row_mul(a, a)
    if mask & OP_CARRY:
        out[2] = R.row_carry(a)
    if mask & OP_POINT:
        out[3] = R.row_double(a)
        out[4] = R.row_add_cached(a, b)
        acc = a
        for _ in range(11):
            acc = R.row_double(acc)
        out[5] = R.row_add_cached(acc, b)
    if mask & OP_SQN:
        out[6] = R.row_sqn(a, 5)
    out[7], out[8] = R.row_bcast01(a)
    out[9], out[10] = R.row_bcast23(a)
    out[11:15] = R.row_bcast_all(a)
    return out


def invert_records(seed=20251018, count=64):
    rng = random.Random(seed)
    pool = K.operands(rng, "tight", 27) + list(NONCANONICAL.values()) + [limbs(1), limbs(2), limbs(P - 2)]
    while len(pool) < count:
        pool.append(limbs(rng.randrange(P)))
    recs = [image(spread([pool] * 4, i, 16)) for i in range(count)]
    recs[0] = image([ZERO_AS_P, [0] * 9, limbs(1), K.TIGHT])           # 0 -> 0 from a zero whose limbs are all non-zero, beside the plain zero
    return recs


def horner_records(seed=20251019):
    """(W, C, top image, W cached images, the W + 1 points or None): real points, then identity / repeated / negated operands, then points with
    raw rows at the edges of the tight class put in (the formulas are polynomial identities, so those need no points behind them)"""
    rng = random.Random(seed)
    edge = K.operands(rng, "tight", 11) + list(NONCANONICAL.values())
    recs = []
    for W, C in HORNER_SHAPES:
        for form in range(4 if (W, C) == (23, 11) else 3):
            pts = [R.random_point(rng) for _ in range(W + 1)]
            rows = [[limbs(v) for v in pts[0]]] + [[limbs(v) for v in cached_of(q)] for q in pts[1:]]
            if form == 1:                                              # identity on top, identity / equal / opposite operands below
                pts[0] = IDENTITY
                for k in range(1, W + 1, 3):
                    pts[k] = IDENTITY
                for k in range(2, W, 5):
                    pts[k + 1] = neg_point(pts[k])
                pts[W] = pts[W - 1]
                rows = [[limbs(v) for v in pts[0]]] + [[limbs(v) for v in cached_of(q)] for q in pts[1:]]
            elif form == 2:                                            # edge rows in the top window and in every operand
                rows = [[edge[(7 * k + 3 * r + W) % 16] if (k + r) % 2 == 0 else rows[k][r] for r in range(4)] for k in range(W + 1)]
            top, cached = image(rows[0]), [image(rw, rng) for rw in rows[1:]]
            recs.append((W, C, top, cached, pts if form != 2 else None))
    return recs


@functools.lru_cache(maxsize=None)
def row_expected():
    """the admitted records and the model's output: (main records, refused records, main images [n][ROW_OPS][64], inversion records, their images,
    Horner records, their images)"""
    main, refused, imgs = [], [], []
    for rec in row_candidates():
        try:
            got = model_images(rec)
        except R.Overflow:
            refused.append(rec)
            continue
        main.append(rec)
        imgs.append(got)
    inv = invert_records()
    inv_imgs = [R.row_invert(a) for a in inv]
    hor = horner_records()
    hor_imgs = [R.row_horner(top, cached, C) for _, C, top, cached, _ in hor]
    return main, refused, np.array(imgs, np.uint32), inv, np.array(inv_imgs, np.uint32), hor, np.array(hor_imgs, np.uint32)


def row_input_words(main, inv, hor):
    """the operand file of row_probe"""
    words = [len(main), len(inv), len(hor), 0]
    for rec in main:
        words += [rec["mask"]] + rec["a"] + rec["b"]
    for a in inv:
        words += a
    for W, C, top, cached, _ in hor:
        assert 1 <= W <= ROW_MAX_W and 1 <= C <= 16 and len(cached) == W
        words += [W, C] + top
        for img in cached:
            words += img
        words += [0] * (64 * (ROW_MAX_W - W))
    return np.array(words, np.uint32)


# ---------------------------------------------------------------------------------------------------------------- quad probe
QUAD_OPS = ["q_double(p)", "q_add_cached(p,s)", "q_add(p,s)", "q_to_cached(p)", "q_load_niels(s) + q_add_cached", "q_load_niels(-s) + q_add_cached"]


@functools.lru_cache(maxsize=None)
def quad_records(seed=20251020):
    """(kind, p rows, s rows): all eight coordinates of the tight class (what quad.h asks of its operands)"""
    rng = random.Random(seed)
    recs = []
    pa = [K.operands(rng, "tight", PER_PAIR) for _ in range(4)]
    pb = [list(reversed(K.operands(rng, "tight", PER_PAIR))) for _ in range(4)]
    for i in range(PER_PAIR):
        recs.append(("tight x tight", spread(pa, i, 24), spread(pb, i, 24)))
    for a_rows, b_rows in edge_pairs("tight", "tight"):
        recs.append(("tight x tight", a_rows, b_rows))
    nc = list(NONCANONICAL.values())
    for i in range(5):
        for j in range(5):
            recs.append(("non-canonical", [nc[(i + r) % 5] for r in range(4)], [nc[(j + 2 * r) % 5] for r in range(4)]))
    for p, q in point_pairs(rng, 16):                                  # the second operand as a point, as its cached form, as its affine niels form
        zi = pow(q[2], P - 2, P)
        x, y = q[0] * zi % P, q[1] * zi % P
        for kind, s in (("points", q), ("points, cached", cached_of(q)), ("points, niels", [(y + x) % P, (y - x) % P, 1, R.D2 * x % P * y % P])):
            recs.append((kind, [limbs(v) for v in p], [limbs(v) for v in s]))
    a = R.random_point(rng)                                            # the identity written with non-canonical zeros and ones, on either side
    recs.append(("points", IDENTITY_AS_P, [limbs(v) for v in a]))
    recs.append(("points", [limbs(v) for v in a], IDENTITY_AS_P))
    return recs


def quad_values(p, s):
    """the six results of a quad record as values, from the formulas over integers"""
    def to_cached(t):
        return cached_of(t)
    dbl = list(R.ext_double(*p))
    return [dbl, add_cached_values(p, s), add_cached_values(p, to_cached(s)), to_cached(p),
            add_cached_values(p, [s[1], s[0], 2, s[3]]), add_cached_values(p, [s[0], s[1], 2, -s[3] % P])]


def quad_input_words(recs):
    return np.array([sum(p, []) + sum(s, []) for _, p, s in recs], np.uint32)


@functools.lru_cache(maxsize=None)
def quad_expected(variant):
    """t_quad_probe of the "plain" or "bound-tracked" host build on quad_records(), in a child process: [n][6][4][9] limbs.  The tracked build
    aborts on a class violation; that is reported as a failure of the calling test."""
    K.build(variant)                                                   # compiled here, loaded there
    recs = quad_records()
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        quad_input_words(recs).tofile(fin)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), variant, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, "t_quad_probe (%s) ended with status %d: %s" % (variant, r.returncode, r.stdout.decode(errors="replace")[-2000:])
        out = np.fromfile(fout, np.uint32)
    assert out.size == len(recs) * 216
    return out.reshape(len(recs), 6, 4, 9)


if __name__ == "__main__":
    variant, fin, fout = sys.argv[1:]
    lib = K.build(variant)
    data = np.fromfile(fin, np.uint32)
    n = data.size // 72
    res = np.zeros(n * 216, np.uint32)
    ub = np.array(K.TIGHT, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.t_quad_probe.restype = None
    lib.t_quad_probe(ctypes.c_uint32(n), data.ctypes.data_as(u32p), ub.ctypes.data_as(u32p), res.ctypes.data_as(u32p))
    res.tofile(fout)

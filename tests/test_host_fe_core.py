"""CPU tests of the field core (fe_mul, fe_sq, fe_sqn, fe_pow22523, fe_invert of zkp_amd/csrc/fe25519.h, host path) against the
formulation it replaced (tests/host/fe_core_host_lib.cpp keeps a copy: columns summed separately, carries rippled afterwards) and
against Python integers, on raw limbs of every input class the header names.  The bound-tracked build is handed the bounds of the
CLASS, so a column or an incoming carry that could overflow for any member of the class aborts the process."""
import ctypes
import random

import pytest

from tests import fe_core_cases as K
from tests import row_quad_cases as C

L9, L8 = ctypes.c_uint32 * 9, ctypes.c_uint32 * 8


@pytest.fixture(scope="module", params=["plain", "bound-tracked"])
def lib(request):
    return K.build(request.param)


def words_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def run_op(lib, op, n, a, ub_a, b, ub_b):
    new, ref, wn, wr = L9(), L9(), L8(), L8()
    tight = lib.t_core_op(op, n, L9(*a), L9(*ub_a), L9(*b), L9(*ub_b), new, ref, wn, wr)
    return tight, list(new), list(ref), words_value(wn), words_value(wr)


def test_admission_rule_matches_the_header():
    """the pairs used below are exactly what the header's vocabulary promises (diff x sum, tight x anything), and the rule refuses the rest"""
    for ca, cb in K.MUL_PAIRS:
        assert K.admits(K.CLASSES[ca], K.CLASSES[cb]), (ca, cb)
    for cls in K.SQ_CLASSES:
        assert K.admits(K.CLASSES[cls], K.CLASSES[cls]), cls
    assert not K.admits(K.CLASSES["diff"], K.CLASSES["diff"]) and not K.admits(K.CLASSES["extreme"], K.CLASSES["sum"])
    assert not K.admits([1 << 31] + [0] * 8, [0] * 9)


def test_mul_against_the_earlier_formulation(lib):
    rng = random.Random(41)
    for ca, cb in K.MUL_PAIRS:
        for a, b in zip(K.operands(rng, ca, 150), reversed(K.operands(rng, cb, 150))):
            tight, new, ref, wn, wr = run_op(lib, 0, 0, a, K.CLASSES[ca], b, K.CLASSES[cb])
            assert tight == 1, (ca, cb, a, b, new)
            assert wn == wr == K.value(a) * K.value(b) % K.P, (ca, cb, a, b)
            assert new == ref, (ca, cb, a, b)                       # the same column values, so the same limbs, not only the same residue


def test_sq_against_the_earlier_formulation(lib):
    rng = random.Random(42)
    for cls in K.SQ_CLASSES:
        for a in K.operands(rng, cls, 300):
            tight, new, ref, wn, wr = run_op(lib, 1, 0, a, K.CLASSES[cls], a, K.CLASSES[cls])
            assert tight == 1, (cls, a, new)
            assert wn == wr == K.value(a) ** 2 % K.P, (cls, a)
            assert new == ref, (cls, a)


def test_squaring_chain_every_count(lib):
    """fe_sqn takes an odd count's first squaring outside its two-per-trip loop: counts 1 .. 12 and the chain's own 20, 50, 100"""
    rng = random.Random(43)
    for cls in K.SQ_CLASSES:
        ops = K.operands(rng, cls, 16)
        for n in list(range(1, 13)) + [20, 50, 100]:
            for a in ops:
                tight, new, ref, wn, wr = run_op(lib, 2, n, a, K.CLASSES[cls], a, K.CLASSES[cls])
                assert tight == 1 and new == ref, (cls, n, a)
                assert wn == wr == pow(K.value(a), 2 ** n, K.P), (cls, n, a)


def test_power_chains_against_integers(lib):
    rng = random.Random(44)
    w = L8()
    for cls in K.SQ_CLASSES:                                        # both chains open with a squaring of their operand
        for a in K.operands(rng, cls, 40):
            v = K.value(a)
            lib.t_core_chain(0, L9(*a), L9(*K.CLASSES[cls]), w)
            assert words_value(w) == pow(v, (K.P - 5) // 8, K.P), (cls, a)
            lib.t_core_chain(1, L9(*a), L9(*K.CLASSES[cls]), w)
            assert words_value(w) == pow(v, K.P - 2, K.P), (cls, a)


@pytest.mark.parametrize("variant", ["plain", "bound-tracked"])
def test_quad_point_arithmetic_lane_by_lane(variant):
    """quad.h's point operations as the host build of the header computes them, a fe per lane and quad.h's calls in quad.h's order
    (t_quad_probe: the reference of tests/test_gpu_row_quad_probe.py), on operands at the edges of the tight class, non-canonical zeros and
    curve points: values against the formulas over Python integers, every output inside the tight class the comments of quad.h promise.  The
    bound-tracked build is given the class maxima as bounds and aborts on a violation (run in a child process: an abort fails this test)."""
    recs = C.quad_records()
    got = C.quad_expected(variant)
    count = {}
    for kind, _, _ in recs:
        count[kind] = count.get(kind, 0) + 1
    assert count == {"tight x tight": 96 + C.EDGE_PAIRS, "non-canonical": 25, "points": 18, "points, cached": 16, "points, niels": 16}
    for (kind, p, s), out in zip(recs, got):
        assert all(l <= t for rows in (p, s) for row in rows for l, t in zip(row, K.TIGHT))
        want = C.quad_values([K.value(r) for r in p], [K.value(r) for r in s])
        for op in range(6):
            assert [K.value([int(x) for x in out[op, q]]) for q in range(4)] == want[op], (kind, C.QUAD_OPS[op])
            assert all(int(out[op, q, k]) <= K.TIGHT[k] for q in range(4) for k in range(9)), (kind, C.QUAD_OPS[op])
        if kind.startswith("points"):                    # ... and where the second operand is a point in the form an operation takes, the sum is one
            op = {"points": 2, "points, cached": 1, "points, niels": 4}[kind]
            for o in (0, op) + ((5,) if op == 4 else ()):
                x, y, z, t = (K.value([int(v) for v in out[o, q]]) for q in range(4))
                assert x * y % K.P == z * t % K.P and (y * y - x * x - z * z - C.R.D * t * t) % K.P == 0 and z, (kind, C.QUAD_OPS[o])
    assert (C.quad_expected("plain") == C.quad_expected("bound-tracked")).all()

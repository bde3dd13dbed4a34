"""CPU tests of the field core (fe_mul, fe_sq, fe_sqn, fe_pow22523, fe_invert of zkp_amd/csrc/fe25519.h, host path) against the
formulation it replaced (tests/host/fe_core_host_lib.cpp keeps a copy: columns summed separately, carries rippled afterwards) and
against Python integers, on raw limbs of every input class the header names.  The bound-tracked build is handed the bounds of the
CLASS, so a column or an incoming carry that could overflow for any member of the class aborts the process."""
import ctypes
import random

import pytest

from tests import fe_core_cases as K

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

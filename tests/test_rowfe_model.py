"""The one-limb-per-lane field and point arithmetic of the Horner tail (zkp_amd/csrc/rowfe.h) as a lane-level model over Python integers
(tools/model/rowfe_model.py: the DPP moves, the column sums, the two carry passes, instruction for instruction): values against big-integer
arithmetic, every intermediate against its register width, outputs inside the "tight" limb class -- the CPU-side half of that file's evidence
(the GPU half: tests/test_gpu_row_quad_probe.py, which pushes the records of tests/row_quad_cases.py through the header on the device and wants
the images this model gives for them, byte for byte; then tests/test_gpu_parity.py::test_row_cooperative_point_ops and every MSM parity test,
whose last kernel is this chain).  The tests at the end of this file check those very images against big integers."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "model"))
import rowfe_model as R  # noqa: E402
from tests import row_quad_cases as C  # noqa: E402


def test_model_matches_integers_and_register_widths():
    assert R.self_check(rounds=120, seed=5)


def test_dpp_moves_are_the_documented_ones():
    v = list(range(100, 164))
    assert R.shr(v, 2)[16 + 5] == v[16 + 3] and R.shr(v, 2)[16 + 1] == 0               # row_shr: zero fill below the row's lane 0
    assert R.shl(v, 7)[32 + 1] == v[32 + 8] and R.shl(v, 7)[32 + 9] == 0               # row_shl: zero fill past the row's lane 15
    assert R.bcast(v, 4)[48 + 11] == v[48 + 4]
    assert R.pull(v, [2, 3, 3, 1])[16 + 7] == v[48 + 7]


def test_multiplication_overflow_is_detected_by_the_model():
    """the width checks are live: operands one class too large must trip them (so that passing means something)"""
    big = [2**32 - 1] * 9
    a = R.rows_of(None, [big] * 4)
    with pytest.raises(R.Overflow):
        R.row_mul(a, a)


def test_identity_and_doubling_through_the_unified_addition():
    rng = random.Random(8)
    ident = (0, 1, 1, 0)
    for _ in range(3):
        p = R.random_point(rng)
        cached = lambda q: R.rows_of([(q[1] - q[0]) % R.P, (q[1] + q[0]) % R.P, 2 * q[2] % R.P, R.D2 * q[3] % R.P])
        for lhs, rhs in ((p, ident), (ident, p), (p, p), (p, (-p[0] % R.P, p[1], p[2], -p[3] % R.P))):
            got = R.row_add_cached(R.rows_of(lhs), cached(rhs))
            vals = tuple(R.value_of(got, r) for r in range(4))
            assert R.same_point(vals, R.ext_add(lhs, rhs))


def test_lane_swaps_of_the_model_are_what_the_hardware_probe_printed():
    """profiles/r05_permlane_probe.txt is the output of tools/microbench/permlane_probe.hip on an MI355X: the model's v_permlane32_swap / v_permlane16_swap
    must give the same source row for every output row (rowfe.h's movement between coordinates rests on exactly these six lines, plus the raw swap16)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = {}
    for line in open(os.path.join(root, "profiles", "r05_permlane_probe.txt")):
        m = re.match(r"(\S+)\s+rows from: (\d) (\d) (\d) (\d)\s+\(lane order inside rows kept\)", line)
        assert m, line
        want[m.group(1)] = [int(g) for g in m.groups()[1:]]
    x = list(range(64))
    rows = lambda v: [v[16 * r] >> 4 for r in range(4)]
    h0, h1 = R.swap32(x, x)
    got = {"swap32(x,x)[0]": rows(h0), "swap32(x,x)[1]": rows(h1)}
    a, b = R.swap16(h0, h0)
    got["swap16(h0,h0)[0]"], got["swap16(h0,h0)[1]"] = rows(a), rows(b)
    a, b = R.swap16(h1, h1)
    got["swap16(h1,h1)[0]"], got["swap16(h1,h1)[1]"] = rows(a), rows(b)
    a, b = R.swap16(x, x)
    got["swap16(x,x)[0]"], got["swap16(x,x)[1]"] = rows(a), rows(b)
    assert got == want
    for v in (h0, h1, a, b):
        assert all(v[16 * r + k] == v[16 * r] + k for r in range(4) for k in range(16))


# ------------------------------------------------------------------------------------------ the records of the device probe through the model
TIGHT = C.K.TIGHT


def assert_tight_image(img, what):
    for r in range(4):
        assert all(int(img[16 * r + k]) <= TIGHT[k] for k in range(9)), ("not tight", what, r)
        assert all(int(img[16 * r + k]) == 0 for k in range(9, 16)), ("idle lanes not zero", what, r)


def test_probe_records_are_admitted_per_class_pair():
    """the model is the admission rule: it refuses the two deliberately inadmissible records and nothing else, so every class pair keeps its count"""
    main, refused = C.row_expected()[:2]
    assert sorted(r["kind"] for r in refused) == ["refused 2^32-1 limbs", "refused diff x diff"]
    count = {}
    for rec in main:
        count[rec["kind"]] = count.get(rec["kind"], 0) + 1
    want = {"mul %s x %s" % pair: C.PER_PAIR + C.EDGE_PAIRS for pair in C.ROW_MUL_PAIRS}
    want.update({"tight x tight": C.PER_PAIR + C.EDGE_PAIRS, "non-canonical": 25, "points": 50, "points with edge rows": 16, "carry 32-bit lanes": 64, "lane index": 1})
    assert count == want and C.PER_PAIR >= 96
    assert len(main) + len(refused) == len(C.row_candidates())
    for rec in main:
        assert all(rec["a"][16 * r + k] == 0 for r in range(4) for k in range(9, 16)) or rec["kind"] == "lane index"
    assert sum(1 for rec in main if any(rec["b"][16 * r + k] for r in range(4) for k in range(9, 16))) >= len(main) - 1    # garbage beside b's limbs
    # the operands really sit at the class edges: every multiplication pair has the two class maxima in one row, and a zero row
    for ca, cb in C.ROW_MUL_PAIRS:
        rows = [(rec["a"][16 * r:16 * r + 9], rec["b"][16 * r:16 * r + 9]) for rec in main if rec["kind"] == "mul %s x %s" % (ca, cb) for r in range(4)]
        assert any(a == C.K.CLASSES[ca] for a, _ in rows) and any(b == C.K.CLASSES[cb] for _, b in rows)
        assert any(a == C.K.CLASSES[ca] and b == C.K.CLASSES[cb] for a, b in rows)                      # ... and the two maxima meet
        assert any(not any(a) for a, _ in rows) and any(not any(b) for _, b in rows)


def test_probe_main_records_against_integers():
    """every image the device will be asked for: its value from big-integer arithmetic on the raw row values (the point formulas are polynomial
    identities, so rows that are no curve point are as good), inside the tight class, zero in the idle lanes"""
    main, _, imgs = C.row_expected()[:3]
    for rec, out in zip(main, imgs):
        a, b, mask, what = C.row_values(rec["a"]), C.row_values(rec["b"]), rec["mask"], rec["kind"]
        vals = [C.row_values([int(x) for x in img]) for img in out]
        for op, on in ((0, C.OP_MUL_AB), (1, C.OP_MUL_AA), (2, C.OP_CARRY), (3, C.OP_POINT), (4, C.OP_POINT), (5, C.OP_POINT), (6, C.OP_SQN)):
            if mask & on:
                assert_tight_image(out[op], (what, C.ROW_OPS[op]))
            else:
                assert not out[op].any()
        if mask & C.OP_MUL_AB:
            assert vals[0] == [x * y % R.P for x, y in zip(a, b)], what
        if mask & C.OP_MUL_AA:
            assert vals[1] == [x * x % R.P for x in a], what
        if mask & C.OP_CARRY:
            assert vals[2] == a, what
        if mask & C.OP_SQN:
            assert vals[6] == [pow(x, 2 ** 5, R.P) for x in a], what
        if mask & C.OP_POINT:
            assert vals[3] == list(R.ext_double(*a)), what
            assert vals[4] == C.add_cached_values(a, b), what
            acc = a
            for _ in range(11):
                acc = R.ext_double(*acc)
            assert vals[5] == C.add_cached_values(acc, b), what
        # the moves between rows: row s of the operand, lane for lane, in front of every row
        for op, src in ((7, 0), (8, 1), (9, 2), (10, 3), (11, 0), (12, 1), (13, 2), (14, 3)):
            assert [int(x) for x in out[op]] == rec["a"][16 * src:16 * src + 16] * 4, (what, C.ROW_OPS[op])


def test_probe_point_records_are_points():
    """the records made of curve points give curve points: 2P, P + Q and 2^11 P + Q projectively, the identity, P = Q and P = -Q among them"""
    main, _, imgs = C.row_expected()[:3]
    seen = 0
    for rec, out in zip(main, imgs):
        if rec["kind"] != "points":
            continue
        seen += 1
        for op in (3, 4, 5):
            x, y, z, t = C.row_values([int(v) for v in out[op]])
            assert x * y % R.P == z * t % R.P and (-x * x + y * y - z * z - R.D * t * t) % R.P == 0 and z != 0
    assert seen == 50


def test_probe_inversions_against_integers():
    _, _, _, inv, imgs = C.row_expected()[:5]
    assert len(inv) == 64
    for a, out in zip(inv, imgs):
        assert_tight_image(out, "row_invert")
        assert C.row_values([int(x) for x in out]) == [pow(v, R.P - 2, R.P) for v in C.row_values(a)]
    assert C.K.value(C.ZERO_AS_P) == 0 and all(C.ZERO_AS_P) and inv[0][:9] == C.ZERO_AS_P      # 0 -> 0 from non-zero limbs


def test_probe_horner_tails_against_the_extended_formulas():
    """the whole chain of k_pip_combine at every (windows, doublings per window) pip_run uses, and the 23 x 11 = 253 doublings of a canonical
    scalar: ext_double / the cached addition over integers, step for step"""
    hor, imgs = C.row_expected()[5:]
    assert sorted({(W, Cb) for W, Cb, _, _, _ in hor}) == sorted(C.HORNER_SHAPES) and len(hor) == 16
    assert set(C.HORNER_SHAPES) == {(-(-256 // c), c) for c in (7, 10, 11, 16)} | {(23, 11)}       # pip_cfg<C>::W for pip_run's four C, and 253 = 23 x 11
    with_points = 0
    for (W, Cb, top, cached, pts), out in zip(hor, imgs):
        acc = C.row_values(top)
        ref = pts and pts[0]
        for k in range(W - 1, -1, -1):
            for _ in range(Cb):
                acc = R.ext_double(*acc)
                ref = ref and R.ext_double(*ref)
            acc = C.add_cached_values(acc, C.row_values(cached[k]))
            ref = ref and R.ext_add(ref, pts[1 + k])
        assert_tight_image(out, ("horner", W, Cb))
        assert C.row_values([int(x) for x in out]) == list(acc), (W, Cb)
        if pts:
            with_points += 1
            assert tuple(acc) == ref, (W, Cb)
    assert with_points == 11

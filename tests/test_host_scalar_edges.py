"""CPU tests of the scalar edge catalogue (tests/scalar_edge_cases.py): the Python restatement of every recoder recombines to the scalar, the
catalogue alone reaches the digits, folds and carries the GPU tests rely on, and the host build of zkp_amd/csrc/sc25519.h computes what
Python integers say for every record of the device probe (tools/microbench/sc_probe.hip) -- so tests/test_gpu_sc_probe.py only has to
compare the device's bytes with expectations proven here."""
import ctypes

import pytest

from tests import scalar_edge_cases as S

L, HALF = S.L, S.HALF
FILL = S.random_256(20251018, 2000)


@pytest.mark.parametrize("name", sorted(S.RECODERS))
def test_model_digits_recombine(name):
    c, rec = S.RECODERS[name]
    lim = 1 << (c - 1)
    for s in S.VALUES + FILL:
        digits, above, fold = rec(s)
        assert fold == (int(HALF < s <= L) if name.startswith("pip") or name == "r16fold" else 0), (name, hex(s))
        assert all(-lim <= d <= lim - 1 for d in digits), (name, hex(s))          # magnitudes in [0, 2^(c-1)], 2^(c-1) only when negative
        assert above in (0, 1), (name, hex(s))
        assert S.recombine(digits, above, c) == (L - s if fold else s), (name, hex(s))


def test_word_models_agree_with_integers():
    for s in S.VALUES + FILL:
        assert S.fold_sign(s) == ((L - s, 1) if HALF < s <= L else (s, 0))
        assert S.not_canonical(s) == int(s >= L)
        for p in S.PROBE_PATTERNS:
            e, top = S.add_pattern(s, p)
            k = sum(p << (32 * i) for i in range(8))
            assert S.from_words(e) + (top << 256) == s + k
    for c in S.PIP_C:                                                            # pip_cfg<C>::kword is the constant K the docstring names
        assert S.from_words([S.pip_kword(c, j) for j in range(9)]) == sum(1 << (c * w + c - 1) for w in range(S.pip_windows(c)))
    assert S.from_words([S.hot_pattern_word(j) for j in range(9)]) == S.from_words([S.pip_kword(7, j) for j in range(9)])


def _coverage(name, values):
    """what the catalogue makes this recoder produce: sets of (window, digit, fold), carries, folds"""
    c, rec = S.RECODERS[name]
    seen = {"win": set(), "above": [], "unfolded_above_l": 0, "l_folds_to_zero": False}
    for s in values:
        digits, above, fold = rec(s)
        seen["above"].append(above)
        for w, d in enumerate(digits):
            seen["win"].add((w, d, fold))
        if s > L and not fold:
            seen["unfolded_above_l"] += 1
        if s == L:
            seen["l_folds_to_zero"] = fold == 1 and not any(digits) and above == 0
    return seen


@pytest.mark.parametrize("c", S.PIP_C)
def test_catalogue_covers_the_pippenger_recoder(c):
    """asserted on the catalogue alone, no random fill"""
    seen = _coverage("pip%d" % c, S.VALUES)
    lo, hi, tf = -(1 << (c - 1)), (1 << (c - 1)) - 1, S.top_full(c)
    for fold in (0, 1):
        assert (0, lo, fold) in seen["win"] and (0, hi, fold) in seen["win"], fold         # both extremes in window 0, with and without the fold
    # ... and in the highest window that can hold them (a partial window above bit 256 - c cannot: its value is below 2^(c-1) + 2^(256 - c W') + 1)
    assert any((tf, lo, f) in seen["win"] for f in (0, 1)) and any((tf, hi, f) in seen["win"] for f in (0, 1))
    assert all(d >= 0 and d < hi for w, d, _ in seen["win"] if w > tf)
    assert seen["unfolded_above_l"] >= 20 and seen["l_folds_to_zero"]
    if c == 16:
        assert sum(seen["above"]) >= 3                                            # the carry window holds a 1
        K = sum(1 << (16 * w + 15) for w in range(16))
        for s, a in zip(S.VALUES, seen["above"]):
            assert a == int(s >= 2**256 - K), hex(s)
        assert {2**256 - K, 2**256 - K - 1, 2**256 - 1} <= set(S.VALUES)
    else:
        assert not any(seen["above"])                                             # pick_c's comment: nothing spills into the carry window
        assert all(S.pip_digits(s, c)[1] == 0 for s in FILL + [2**256 - 1])


@pytest.mark.parametrize("name", ["hot", "r16", "r16fold", "r4", "r256"])
def test_catalogue_covers_the_other_recoders(name):
    c, _ = S.RECODERS[name]
    seen = _coverage(name, S.VALUES)
    lo, hi, tf = -(1 << (c - 1)), (1 << (c - 1)) - 1, S.top_full(c)
    folds = (0, 1) if name == "r16fold" else (0,)
    for fold in folds:
        assert (0, lo, fold) in seen["win"] and (0, hi, fold) in seen["win"], fold
    assert any((tf, lo, f) in seen["win"] for f in folds) and any((tf, hi, f) in seen["win"] for f in folds)
    assert seen["unfolded_above_l"] >= 20
    if name == "hot":
        assert not any(seen["above"])                                             # hot_tables.h: e < 2^(7 * 37), nothing is left after the last window
    else:
        assert sum(seen["above"]) >= 3
        K = sum(1 << (c * w + c - 1) for w in range(256 // c))
        if name == "r16fold":
            assert seen["l_folds_to_zero"]
        for s, a in zip(S.VALUES, seen["above"]):
            assert a == int(s >= 2**256 - K), hex(s)                              # (a folded value is below 2^252: no carry)
        assert {2**256 - K, 2**256 - K - 1, 2**256 - 1} <= set(S.VALUES)


def test_probe_records_hold_the_montgomery_cases():
    recs = S.probe_records()
    cat = set(S.VALUES)
    assert len(recs) >= 4000 and sum(1 for a, b, _ in recs if a in cat and b in cat) >= 2000
    n_hi = n_lo = n_m0 = 0
    for a, b, _ in recs:
        r, pre, col, m0 = S.mont_trace(a, b % L)
        assert r == a * (b % L) * pow(2, -256, L) % L
        n_hi += pre >= L
        n_lo += pre < L
        n_m0 += m0 > 0
        # the column t[8] = t[9] + carry that a round leaves behind: with b < l the running value stays below 2 l + l / 2^32 < 2^254 after
        # every round, so the column is 0 for EVERY first operand -- the all-ones words included
        assert col == 0
    # the final conditional subtraction fires in a good share of the records and stays idle in another; some rounds have m = 0
    assert n_hi >= len(recs) // 20 and n_lo >= len(recs) // 4, (n_hi, n_lo)
    assert n_m0 >= 20, n_m0
    assert (2**256 - 1, L - 1, L - 1) in recs and any(a == 0 for a, _, _ in recs)
    q = (2**512 - 1) // L * L
    wide = {a + (b << 256) for a, b, _ in recs}
    assert {0, L, 2**256, 2**256 + L, L << 256, 2**512 - 1, q, q - 1} <= wide


def test_host_build_of_the_header_on_the_probe_records():
    """every output of the probe, computed by the host build of sc25519.h (tests/host/fe_host_lib.cpp: t_sc_op), against Python integers"""
    from tests.test_host_field import _build
    lib = _build("plain")
    out = ctypes.create_string_buffer(32)
    b32 = lambda x: x.to_bytes(32, "little")

    def op(k, x, y=b32(0)):
        flag = lib.t_sc_op(k, x, y, out)
        return S.words(int.from_bytes(out.raw, "little")), flag

    for a, b, c in S.probe_records():
        want = S.probe_expected(a, b, c)
        A, B, C = b32(a), b32(b), b32(c)
        ar, _ = op(3, A)
        br, _ = op(3, B)
        cr, _ = op(3, C)
        Ar, Br, Cr = (b32(S.from_words(w)) for w in (ar, br, cr))
        got = list(ar)
        got += op(8, A)[0] + op(9, A, Br)[0] + op(0, A, Br)[0] + op(1, Ar, Br)[0] + op(2, Ar)[0] + op(5, A, B)[0] + op(7, A)[0] + op(10, Ar)[0]
        folded, flag = op(16, A)
        got += folded + [flag, op(11, A)[1]] + [0] * 6
        tops = []
        for k in (12, 13, 14):
            e, top = op(k, A)
            got += e
            tops.append(top)
        got += tops + [0] * 5
        got += op(15, A, Br + Cr)[0]
        assert got == want, (hex(a), hex(b), hex(c), [i // 8 for i in range(128) if got[i] != want[i]][:4])

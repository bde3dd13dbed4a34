"""Reduced scalars at the edges of the sign-folded radix-16 recoding (zkp_amd/csrc/sc25519.h: sc_fold_recode16), shared by
tests/test_host_comb_fold.py and tests/test_gpu_comb_fold.py.

The walks take f = min(s, l - s) <= (l - 1) / 2 as e = f + K62, K62 = sum_{i < 62} 8 * 16^i: nibbles 0 .. 61 of e are the signed digits
nibble - 8, e >> 248 is the digit of nibble 62 as it stands (0 .. 8), nibble 63 does not exist."""
from oracle import model as M

L = M.L
HALF = (L - 1) // 2
K62 = sum(8 << (4 * i) for i in range(62))
TOP = 62                                        # the nibble whose digit carries no offset


def fold(s):
    """-> (f, flip) as sc_fold_sign gives them for a value that is at most l"""
    return (L - s, 1) if HALF < s <= L else (s, 0)


def digits(f):
    """the 63 digits of the folded recoding of f, lowest first (the last one as it stands)"""
    e = f + K62
    assert e >> 252 == 0
    return [((e >> (4 * i)) & 15) - 8 for i in range(TOP)] + [e >> (4 * TOP)]


def _digit(n, d):
    return (d << (4 * n)) % L


def catalogue():
    cat = [0, 1, HALF, HALF + 1, L - 1, 2**251 - 1, 2**251, 2**251 + 1, 2**248 - 1, 2**248]
    cat += [2**248 - K62 - 1, 2**248 - K62, 2**248 - K62 + 1]                  # around the first carry into nibble 62
    for n in (0, 15, 16, 47, 60, 61):
        for d in (8, 7, -7, -8):
            cat.append(_digit(n, d))
    cat += [_digit(TOP, 7), _digit(TOP, 8)]                                     # raw 7 and 8 in nibble 62
    out = []
    for v in cat:
        for s in (v, (L - v) % L):                                             # each entry as s and as l - s
            assert 0 <= s < L
            if s not in out:
                out.append(s)
    return out


CAT = catalogue()

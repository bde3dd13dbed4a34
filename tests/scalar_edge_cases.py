"""(helper module of tests/test_host_scalar_edges.py, tests/test_gpu_scalar_edges.py and tests/test_gpu_sc_probe.py)
256-bit scalars at the edges of every signed-digit recoder of the library, and the recoders restated in Python.

include/zkp_mi355x.h promises that the MSM entry points take any 256-bit string as an integer multiplier.  Every recoder adds a constant
K = sum_w 2^(c w + c - 1) to the scalar and reads c-bit windows of the sum: digit_w = window_w - 2^(c-1) in [-2^(c-1), 2^(c-1) - 1], no
sequential carry.  What is left above the last window is the "carry window" of the Pippenger path (k_pip_prepare) or the carry-out `top` of
sc_add_pattern.  The recoders:

  name     c    kernel code                                          fold   above the windows
  pip7     7    k_pip_prepare<7>                                     yes    carry window 37 (bit 259): 0 for every 256-bit scalar
  pip10   10    k_pip_prepare<10>                                    yes    carry window 26 (bit 260): 0
  pip11   11    k_pip_prepare<11>                                    yes    carry window 24 (bit 264): 0
  pip16   16    k_pip_prepare<16>                                    yes    carry window 16 (bit 256): 1 iff s >= 2^256 - K
  hot      7    hot_recode / hot_next_digit (hot_tables.h)           no     none (37 windows reach bit 259)
  r16      4    sc_add_pattern(0x88888888) + nibbles (comb_tables.h) no*    top = 1 iff s >= 2^256 - K
  r4       2    sc_add_pattern(0xAAAAAAAA) + bit pairs (term_generic) no    top
  r256     8    sc_add_pattern(0x80808080) + bytes (the rider)       no     top
  (* the Straus walk of fused_flows.h folds before it recodes: radix_digits(..., fold=True))

Sign folding (sc_fold_sign): (l-1)/2 < s <= l is replaced by l - s and the digits change sign; s > l is left alone.

CATALOGUE is a list of (name, value), values distinct.  The constructions per recoder, in terms of digits (top_full = the highest window
whose c bits all lie below bit 256; a 256-bit scalar cannot put either extreme digit into a partial window above it):
  allmin    digit -2^(c-1) in every window a 256-bit scalar can put it in: windows 0 .. top_full.  Above them the partial window holds its
            largest digit, so that the value exceeds l and reaches the recoder unfolded; for c | 256 there is none: window top_full gets +1,
            and all 256/c windows at -2^(c-1) is carry_min below
  allmax    digit 2^(c-1) - 1 in windows 0 .. top_full (the partial window as in allmin)
  alt       the two extremes alternating, 2^(c-1) - 1 in window top_full;   alt2: the other phase, -2^(c-1) on top
  top       one non-zero digit, the largest the highest window can hold
  bot_max   2^(c-1) - 1: one non-zero digit in window 0          bot_min   2^(c-1): digit -2^(c-1) in window 0 under a +1 in window 1
  *_low     allmin, allmax, alt and alt2 over the windows below bit 251 only: these values are below (l-1)/2
  carry_min, carry_max, carry_below (c | 256 only)   2^256 - K, 2^256 - 1, 2^256 - K - 1
and l - v for every constructed v <= (l-1)/2: the fold fires and the recoder sees v.
"""
import random

L = 2**252 + 27742317777372353535851937790883648493
HALF = (L - 1) // 2
M256 = 2**256 - 1
M32 = 0xFFFFFFFF

PIP_C = (7, 10, 11, 16)
HOT_W = 7
PATTERNS = {"r16": (4, 0x88888888), "r4": (2, 0xAAAAAAAA), "r256": (8, 0x80808080)}      # name: (digit bits, word pattern of K)


def words(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---- the device code, word by word ---------------------------------------------------------------------------------------------------------
def fold_sign(s):
    """sc_fold_sign: two borrow chains over eight words -> (value the recoder sees, fold flag)"""
    sw, hw, lw = words(s), words(HALF), words(L)
    d, b1, b2 = [0] * 8, 0, 0
    for i in range(8):
        t1 = (hw[i] - sw[i] - b1) & (2**64 - 1)
        b1 = (t1 >> 63) & 1
        t2 = (lw[i] - sw[i] - b2) & (2**64 - 1)
        d[i] = t2 & M32
        b2 = (t2 >> 63) & 1
    fold = bool(b1 and not b2)
    return (from_words(d) if fold else s), int(fold)


def not_canonical(s):
    """sc_not_canonical: 1 iff the borrow chain of s - l ends without a borrow"""
    sw, lw, br = words(s), words(L), 0
    for i in range(8):
        br = (((sw[i] - lw[i] - br) & (2**64 - 1)) >> 63) & 1
    return 0 if br else 1


def add_pattern(s, pattern):
    """sc_add_pattern -> (e as eight words, top)"""
    sw, e, c = words(s), [0] * 8, 0
    for i in range(8):
        c += sw[i] + pattern
        e[i] = c & M32
        c >>= 32
    return e, c


def pip_windows(c):
    return (256 + c - 1) // c


def pip_kword(c, j):
    """pip_cfg<C>::kword"""
    r = 0
    for w in range(pip_windows(c)):
        bit = c - 1 + c * w
        if bit // 32 == j:
            r |= 1 << (bit % 32)
    return r


def _signed(v, c):
    """window value -> (magnitude, neg) as the kernels split it"""
    half = 1 << (c - 1)
    neg = int(v < half)
    return (half - v if neg else v - half), neg


def pip_digits(s, c):
    """k_pip_prepare<c>: (signed digits of the W offset windows, carry window, fold flag).  The digits are those of the value after
    folding: sum digit_w 2^(c w) + carry 2^(c W) = s, or l - s when folded (the kernel then flips every sign bit)."""
    W = pip_windows(c)
    v, fold = fold_sign(s)
    sw = words(v)
    e, cy = [0] * 10, 0
    for j in range(9):
        cy += (sw[j] if j < 8 else 0) + pip_kword(c, j)
        e[j] = cy & M32
        cy >>= 32
    digits = []
    for w in range(W + 1):
        pos = c * w
        lo, sh = pos >> 5, pos & 31
        x = e[lo] >> sh
        if sh + c > 32:
            x |= (e[lo + 1] << (32 - sh)) & M32
        x &= (1 << c) - 1
        if w < W:
            mag, neg = _signed(x, c)
            assert 0 <= mag <= 1 << (c - 1)
            digits.append(-mag if neg else mag)
        else:
            carry = x
    return digits, carry, fold


def radix_digits(s, pattern, fold=False):
    """sc_add_pattern(s, pattern) and the split into nibbles (0x88888888), bytes (0x80808080) or bit pairs (0xAAAAAAAA), lowest digit
    first -> (signed digits, top, fold flag); fold=True: sc_fold_sign first, as the Straus walk of fused_flows.h does"""
    c = {0x88888888: 4, 0x80808080: 8, 0xAAAAAAAA: 2}[pattern]
    v, f = fold_sign(s) if fold else (s, 0)
    e, top = add_pattern(v, pattern)
    digits = []
    for j in range(8):
        cur = e[j]
        for _ in range(32 // c):
            mag, neg = _signed(cur & ((1 << c) - 1), c)
            cur >>= c
            digits.append(-mag if neg else mag)
    return digits, top, f


HOT_WINDOWS = (257 + HOT_W - 1) // HOT_W


def hot_pattern_word(i):
    v = 0
    for w in range(HOT_WINDOWS):
        bit = HOT_W * w + HOT_W - 1
        if bit // 32 == i:
            v |= 1 << (bit % 32)
    return v


def hot_digits(s):
    """hot_recode, then HOT_WINDOWS times hot_next_digit -> (signed digits, what is left of e (0 for every 256-bit scalar), fold flag 0)"""
    sw, e, c = words(s), [0] * 9, 0
    for i in range(8):
        c += sw[i] + hot_pattern_word(i)
        e[i] = c & M32
        c >>= 32
    e[8] = (c + hot_pattern_word(8)) & M32
    digits = []
    for _ in range(HOT_WINDOWS):
        d = e[0] & ((1 << HOT_W) - 1)
        for i in range(8):                                   # v_alignbit(e[i + 1], e[i], HOT_W)
            e[i] = ((e[i] >> HOT_W) | (e[i + 1] << (32 - HOT_W))) & M32
        e[8] >>= HOT_W
        mag, neg = _signed(d, HOT_W)
        digits.append(-mag if neg else mag)
    return digits, from_words(e), 0


RECODERS = {"pip7": (7, lambda s: pip_digits(s, 7)), "pip10": (10, lambda s: pip_digits(s, 10)), "pip11": (11, lambda s: pip_digits(s, 11)),
            "pip16": (16, lambda s: pip_digits(s, 16)), "hot": (HOT_W, hot_digits),
            "r16": (4, lambda s: radix_digits(s, 0x88888888)), "r16fold": (4, lambda s: radix_digits(s, 0x88888888, fold=True)),
            "r4": (2, lambda s: radix_digits(s, 0xAAAAAAAA)), "r256": (8, lambda s: radix_digits(s, 0x80808080))}


def recombine(digits, above, c):
    """the integer a digit vector stands for: sum digit_w 2^(c w) + above 2^(c len(digits))"""
    return sum(d << (c * w) for w, d in enumerate(digits)) + (above << (c * len(digits)))


def top_full(c):
    """the highest window whose c bits all lie below bit 256"""
    return 256 // c - 1


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------
def _constructions(c):
    lo, hi = -(1 << (c - 1)), (1 << (c - 1)) - 1
    tf = top_full(c)
    exact = 256 % c == 0
    from_digits = lambda ds: sum(d << (c * w) for w, d in enumerate(ds))
    out = []
    if exact:
        out.append(("allmin", from_digits([lo] * tf + [1])))
        out.append(("top", hi << (c * tf)))
    else:
        ptop = (1 << (256 - c * (tf + 1))) - 1               # the largest digit of the partial window: with it the value exceeds l (no fold)
        out.append(("allmin", from_digits([lo] * (tf + 1) + [ptop])))
        out.append(("top", ptop << (c * (tf + 1))))
    out.append(("allmax", from_digits([hi] * (tf + 1) + ([] if exact else [ptop]))))
    out.append(("alt", from_digits([hi if (tf - w) % 2 == 0 else lo for w in range(tf + 1)] + ([] if exact else [ptop]))))
    if exact:                                                # the other phase: -2^(c-1) on top of the alternation, a +1 above it
        out.append(("alt2", from_digits([lo if (tf - 1 - w) % 2 == 0 else hi for w in range(tf)] + [1])))
    else:
        out.append(("alt2", from_digits([lo if (tf - w) % 2 == 0 else hi for w in range(tf + 1)] + [ptop])))
    out.append(("bot_max", hi))
    out.append(("bot_min", 1 << (c - 1)))
    m = 251 // c                                             # windows 0 .. m - 1 lie below bit 251
    out.append(("allmin_low", from_digits([lo] * m + [1])))
    out.append(("allmax_low", from_digits([hi] * m)))
    out.append(("alt_low", from_digits([hi if (m - 1 - w) % 2 == 0 else lo for w in range(m)])))
    out.append(("alt2_low", from_digits([lo if (m - 1 - w) % 2 == 0 else hi for w in range(m)] + [1])))
    if exact:
        K = sum(1 << (c * w + c - 1) for w in range(256 // c))
        out += [("carry_min", 2**256 - K), ("carry_max", 2**256 - 1), ("carry_below", 2**256 - K - 1)]
    return out


def _catalogue():
    cat = [("0", 0), ("1", 1), ("2", 2), ("half-1", HALF - 1), ("half", HALF), ("half+1", HALF + 1), ("l-2", L - 2), ("l-1", L - 1), ("l", L),
           ("l+1", L + 1), ("l+2", L + 2)]
    cat += [("%dl%+d" % (k, d) if d else "%dl" % k, k * L + d) for k in (2, 8, 15) for d in (-1, 0, 1)]
    cat += [("2^128-1", 2**128 - 1), ("2^128", 2**128), ("l-(2^128-1)", L - (2**128 - 1)), ("2^252-1", 2**252 - 1), ("2^252", 2**252),
            ("2^253-1", 2**253 - 1), ("2^253", 2**253), ("2^254", 2**254), ("2^255-1", 2**255 - 1), ("2^255", 2**255), ("2^255+1", 2**255 + 1),
            ("2^256-2^128", 2**256 - 2**128), ("2^256-2", 2**256 - 2), ("2^256-1", 2**256 - 1)]
    recs = [("pip%d" % c, c) for c in PIP_C] + [("hot", HOT_W)] + [(k, v[0]) for k, v in PATTERNS.items()]
    for rname, c in recs:
        for cname, v in _constructions(c):
            assert 0 <= v < 2**256, (rname, cname)
            cat.append(("%s:%s" % (rname, cname), v))
            if v <= HALF:                                    # l - v lies in (half, l]: folded, the recoder sees v
                cat.append(("l-%s:%s" % (rname, cname), L - v))
    seen, out = {}, []
    for name, v in cat:                                      # (pip7 and hot share K; small constructions meet the fold boundary list)
        if v in seen:
            out[seen[v]] = (out[seen[v]][0] + "=" + name, v)
        else:
            seen[v] = len(out)
            out.append((name, v))
    return out


CATALOGUE = _catalogue()
VALUES = [v for _, v in CATALOGUE]
assert 130 <= len(CATALOGUE) <= 170 and all(0 <= v < 2**256 for v in VALUES) and len(set(VALUES)) == len(VALUES)


def random_256(seed, count):
    rng = random.Random(seed)
    return [rng.getrandbits(256) for _ in range(count)]


# ---- records of the scalar probe (tools/microbench/sc_probe.hip) -----------------------------------------------------------------------------
RR = pow(2, 512, L)
N0INV = (-pow(L, -1, 2**32)) % 2**32
PROBE_PATTERNS = (0x88888888, 0xAAAAAAAA, 0x80808080)
PROBE_OUT_WORDS = 16 * 8                                     # per record: see probe_expected


def mont_trace(a, b):
    """sc_mont(a, b) word by word -> (result, value before the final conditional subtraction, largest t[9] + carry column seen, rounds with m = 0)"""
    aw, bw, lw = words(a), words(b), words(L)
    t = [0] * 10
    col, m0 = 0, 0
    for i in range(8):
        c = 0
        for j in range(8):
            c += aw[i] * bw[j] + t[j]
            t[j] = c & M32
            c >>= 32
        c += t[8]
        t[8] = c & M32
        t[9] = c >> 32
        m = (t[0] * N0INV) & M32
        m0 += m == 0
        c = (m * lw[0] + t[0]) >> 32
        for j in range(1, 8):
            c += m * lw[j] + t[j]
            t[j - 1] = c & M32
            c >>= 32
        c += t[8]
        t[7] = c & M32
        t[8] = t[9] + (c >> 32)
        assert t[8] <= M32
        col = max(col, t[8])
    pre = from_words(t[:8])
    assert t[8] == 0 and pre < 2 * L
    return (pre - L if pre >= L else pre), pre, col, m0


def probe_records(seed=20251018):
    """(a, b, c) triples of 256-bit values: the catalogue crossed with itself on a seeded subset, the Montgomery- and wide-specific operands of
    the issue, random records"""
    rng = random.Random(seed)
    recs = []
    for _ in range(2200):
        recs.append((rng.choice(VALUES), rng.choice(VALUES), rng.choice(VALUES)))
    for a in VALUES:                                         # every catalogue value as first operand at least once, against itself too
        recs.append((a, a, rng.choice(VALUES)))
    recs.append((M256, L - 1, L - 1))
    for i in range(8):
        recs.append((M32 << (32 * i), rng.choice(VALUES), rng.getrandbits(256)))
        recs.append((M32 << (32 * i), L - 1, L - 1))
    recs.append((0, rng.getrandbits(256), rng.getrandbits(256)))
    for k in range(1, 8):                                    # multiples of 2^32 (2^(32 k)): m = 0 in the first k rounds
        recs.append((rng.getrandbits(256 - 32 * k) << (32 * k), rng.getrandbits(256), rng.getrandbits(256)))
    # pairs whose first Montgomery product ends in [l, 2l) before the subtraction, and pairs that end below l: found with the model
    hi, lo = [], []
    while len(hi) < 150 or len(lo) < 150:
        a, b = rng.getrandbits(256), rng.getrandbits(256)
        _, pre, _, _ = mont_trace(a, b % L)
        (hi if pre >= L else lo).append((a, b, rng.getrandbits(256)))
    recs += hi[:150] + lo[:150]
    q = (2**512 - 1) // L * L
    for x in (0, L, 2**256, 2**256 + L, L << 256, 2**512 - 1, q, q - 1):      # wide values: a = low half, b = high half
        recs.append((x & M256, x >> 256, rng.getrandbits(256)))
    for _ in range(2000):
        recs.append((rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)))
    return recs


def probe_expected(a, b, c):
    """the 128 output words of one record, from Python integers.  b' = b mod l, c' = c mod l, a' = a mod l (the probe reduces them itself)."""
    ar, br, cr = a % L, b % L, c % L
    rinv = pow(2, -256, L)
    folded, flag = ((L - a), 1) if HALF < a <= L else (a, 0)
    vals = [ar, a * 2**256 % L, a * br * rinv % L, a * br % L, (ar + br) % L, (-ar) % L, (a + (b << 256)) % L, a * ((L + 1) // 2) % L,
            ar * ((L + 1) // 2) % L, folded]
    out = []
    for v in vals:
        out += words(v)
    out += [flag, int(a >= L), 0, 0, 0, 0, 0, 0]
    tops = []
    for p in PROBE_PATTERNS:
        k = sum(p << (32 * i) for i in range(8))
        out += words((a + k) & M256)
        tops.append((a + k) >> 256)
    out += tops + [0] * 5
    out += words((a * cr + br) % L)
    assert len(out) == PROBE_OUT_WORDS
    return out

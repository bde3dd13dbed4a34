"""Operands for the field-core tests (tests/test_host_fe_core.py, tests/test_gpu_fe_core.py): raw 9 x 29-bit limbs of every input class
zkp_amd/csrc/fe25519.h names, with the class bounds the bound tracker is given, and the tracker's admission rule restated in Python
so that a test never hands the tracked build a pair it would abort on."""
import ctypes
import os
import random
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "fe_core_host_lib.cpp")

P = 2 ** 255 - 19
TIGHT = [(1 << 29) + (1 << 18) - 1] * 8 + [(1 << 23) + (1 << 4) - 1]            # inclusive maxima of the "tight" class
BIAS2P = [0x3fffffda] + [0x3ffffffe] * 7 + [0x00fffffe]
CLASSES = {
    "tight": TIGHT,
    "sum": [2 * t for t in TIGHT],                                                # tight + tight
    "diff": [t + b for t, b in zip(TIGHT, BIAS2P)],                               # tight + 2p - tight
    "extreme": [(1 << 31) - 1] * 9,                                               # the largest limbs fe_track_mul admits at all
}


def value(limbs):
    return sum(l << (29 * i) for i, l in enumerate(limbs)) % P


def admits(ub_a, ub_b):
    """fe_track_mul's rule: limbs < 2^31, every high column < 2^64, every low column + folds + the 2^36 carry allowance < 2^64"""
    if max(ub_a) >= 1 << 31 or max(ub_b) >= 1 << 31:
        return False
    col = [0] * 17
    for i in range(9):
        for j in range(9):
            col[i + j] += ub_a[i] * ub_b[j]
    lim = (1 << 64) - 1
    if any(c > lim for c in col[9:]):
        return False
    for k in range(9):
        t = col[k] + (1216 * 0xffffffff if k <= 7 else 0) + (9728 * 0xffffffff if k >= 1 else 0) + (1 << 36)
        if t > lim:
            return False
    return True


def operands(rng, cls, count):
    """count limb vectors of class cls: the class maximum, all zero, one limb at its maximum, then uniformly random limbs"""
    ub = CLASSES[cls]
    out = [list(ub), [0] * 9] + [[ub[i] if i == j else 0 for i in range(9)] for j in range(9)]
    while len(out) < count:
        out.append([rng.randrange(u + 1) for u in ub])
    return out[:count]


MUL_PAIRS = [("tight", "tight"), ("tight", "sum"), ("sum", "tight"), ("sum", "sum"), ("diff", "sum"), ("sum", "diff"), ("tight", "diff"),
             ("diff", "tight"), ("extreme", "tight"), ("tight", "extreme")]
SQ_CLASSES = ["tight", "sum"]


def probe_records(seed=20250707, per_pair=96):
    """(limbs a, limbs b, bounds a, bounds b) for the probe kernel: a is squared too, so a is tight or sum"""
    rng = random.Random(seed)
    recs = []
    for ca, cb in MUL_PAIRS:
        if ca not in SQ_CLASSES:
            continue
        for a, b in zip(operands(rng, ca, per_pair), reversed(operands(rng, cb, per_pair))):
            recs.append((a, b, CLASSES[ca], CLASSES[cb]))
    return recs


def build(variant):
    """tests/host/fe_core_host_lib.cpp as a shared library: "plain" or "bound-tracked" (-DZKP_FE_TRACK)"""
    out = os.path.join(HERE, "host", {"plain": "fe_core_host_lib.so", "bound-tracked": "fe_core_host_lib_track.so"}[variant])
    deps = [SRC] + [os.path.join(HERE, "..", "zkp_amd", "csrc", f) for f in ("fe25519.h", "fe_constants.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SRC, "-o", out]
        if variant == "bound-tracked":
            cmd.insert(1, "-DZKP_FE_TRACK")
        subprocess.check_call(cmd)
    lib = ctypes.CDLL(out)
    assert lib.t_core_tracked() == int(variant == "bound-tracked")
    return lib

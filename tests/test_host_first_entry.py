"""CPU tests of ge_from_niels / ge_from_cached (zkp_amd/csrc/ge25519.h): the walks set their accumulator from the first table entry
instead of adding that entry onto the identity.  The helpers are compiled for the host from the header the kernels compile -- plain,
with the interval bound tracker (-DZKP_FE_TRACK aborts on any possible overflow for the whole limb class), and over the host backend's
5 x 51-bit field -- and compared with the addition they replace and with the big-integer model (oracle/model.py)."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "first_entry_host_lib.cpp")
D_INV = pow(M.D, M.P - 2, M.P)


def _build(variant: str):
    out = os.path.join(HERE, "host", {"plain": "first_entry_host_lib.so", "bound-tracked": "first_entry_host_lib_track.so",
                                      "host-fe51": "first_entry_host_lib_fe51.so"}[variant])
    deps = [SRC] + [os.path.join(HERE, "..", "zkp_amd", "csrc", f) for f in ("fe25519.h", "ge25519.h", "fe_constants.h", os.path.join("host", "fe51.h"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SRC, "-o", out]
        if variant == "bound-tracked":
            cmd.insert(1, "-DZKP_FE_TRACK")
        if variant == "host-fe51":
            cmd.insert(1, "-DZKP_HOST_FE51")
        subprocess.check_call(cmd)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module", params=["plain", "bound-tracked", "host-fe51"])
def lib(request):
    return _build(request.param)


def _shape(lib):
    """(limbs per element, bits per limb, inclusive maxima of the tight class)"""
    nl = lib.t_limbs()
    if nl == 5:
        return nl, 51, [(1 << 51) + (1 << 14) - 1] * 5
    return nl, 29, [(1 << 29) + (1 << 18)] * 8 + [(1 << 23) + 16]


def _limbs(lib, x):
    nl, bits, _ = _shape(lib)
    x %= M.P
    return [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(nl)]


def _value(lib, limbs):
    _, bits, _ = _shape(lib)
    return sum(l << (bits * i) for i, l in enumerate(limbs)) % M.P


def _run(lib, form, cneg, neg, fields):
    flat = [l for f in fields for l in f]
    xyzt = ctypes.create_string_buffer(128)
    encs = ctypes.create_string_buffer(64)
    lib.t_first_entry(form, cneg, neg, (ctypes.c_uint64 * len(flat))(*flat), xyzt, encs)
    return [int.from_bytes(xyzt.raw[32 * k:32 * k + 32], "little") for k in range(4)], encs.raw[:32], encs.raw[32:]


def _model(form, cneg, neg, vals):
    """the helper's coordinates from the entry's field values"""
    if form == 0:
        ypx, ymx, t = vals
        z = 2
    else:
        ypx, ymx, z, t = vals
    if cneg:
        ypx, ymx, t = ymx, ypx, -t
    if neg:
        ypx, ymx, t = ymx, ypx, -t
    return [(ypx - ymx) % M.P, (ypx + ymx) % M.P, z % M.P, t * D_INV % M.P]


def _entry(point, form, z=1):
    x, y, pz, _ = point
    zi = pow(pz, M.P - 2, M.P)
    x, y = x * zi % M.P, y * zi % M.P
    if form == 0:
        return [(y + x) % M.P, (y - x) % M.P, 2 * M.D * x * y % M.P]
    return [(y + x) * z % M.P, (y - x) * z % M.P, 2 * z % M.P, 2 * M.D * x * y * z % M.P]


@pytest.mark.parametrize("form", [0, 1], ids=["niels", "cached"])
def test_first_entry_is_identity_plus_entry(lib, form):
    rng = random.Random(81 + form)
    points = [M.IDENTITY, M.BASEPOINT, M.pt_neg(M.BASEPOINT)]
    for _ in range(24):
        p = M.pt_mul(rng.randrange(1, M.L), M.BASEPOINT)
        points += [p, M.pt_neg(p)]                                  # entries and their negations
    for p in points:
        z = 1 if p is M.BASEPOINT else rng.randrange(1, M.P)
        vals = _entry(p, form, z)
        for cneg in (0, 1):
            for neg in (0, 1):
                got, enc_helper, enc_add = _run(lib, form, cneg, neg, [_limbs(lib, v) for v in vals])
                want = M.ristretto_encode(M.pt_neg(p) if cneg ^ neg else p)
                assert enc_helper == enc_add == want, (form, cneg, neg, p)
                assert got == _model(form, cneg, neg, vals), (form, cneg, neg, p)


@pytest.mark.parametrize("form", [0, 1], ids=["niels", "cached"])
def test_identity_entry(lib, form):
    """a zero digit is masked to the identity entry (1, 1, 0) / (1, 1, 2, 0): its conversion is (0, 2, 2, 0), the identity"""
    vals = [1, 1, 0] if form == 0 else [1, 1, 2, 0]
    for cneg in (0, 1):
        for neg in (0, 1):
            got, enc_helper, enc_add = _run(lib, form, cneg, neg, [_limbs(lib, v) for v in vals])
            assert got == [0, 2, 2, 0]
            assert enc_helper == enc_add == M.IDENTITY_ENC


@pytest.mark.parametrize("form", [0, 1], ids=["niels", "cached"])
def test_limbs_at_class_maxima(lib, form):
    """every limb of every element at the maximum of the tight class, at zero, and mixed: the coordinates are those of the model (such
    entries are not curve points, so there is no encoding to compare; the bound-tracked build checks the class whatever the values)"""
    nl, _, mx = _shape(lib)
    rng = random.Random(83 + form)
    nf = 3 if form == 0 else 4
    cases = [[mx] * nf, [[0] * nl] * nf]
    for k in range(nf):
        cases.append([mx if i == k else [0] * nl for i in range(nf)])
        cases.append([[0] * nl if i == k else mx for i in range(nf)])
    for _ in range(60):
        cases.append([[rng.choice((0, 1, m - 1, m, rng.randrange(m + 1))) for m in mx] for _ in range(nf)])
    for fields in cases:
        vals = [_value(lib, f) for f in fields]
        for cneg in (0, 1):
            for neg in (0, 1):
                got, _, _ = _run(lib, form, cneg, neg, fields)
                assert got == _model(form, cneg, neg, vals), (form, cneg, neg, fields)

"""Every MSM path at the edges of 256-bit scalars (tests/scalar_edge_cases.py): include/zkp_mi355x.h promises that the MSM entry points use any
256-bit string as an integer multiplier, and before this file only zkp_msm_many had met l, l + 5, 2^255 and 2^256 - 1.  Here the Pippenger
path behind zkp_msm_optional[_dev] sees the whole catalogue at every window size -- the extreme digits -2^(c-1) and 2^(c-1) - 1 in the
bottom and top windows, the sign fold at its boundary, l itself, unfolded values above l, and for c = 16 the carry window, which holds a 1
exactly when s >= 2^256 - K and had never held one in any test -- and zkp_msm_many sees it on every class of point.

The reference is exact: all points are k_j * B with known k_j, so a call must return ristretto_encode(((sum s_i k_j(i)) mod l) * B) of
oracle/model.py with s_i taken as the plain 256-bit integer.  Byte for byte, no tolerance."""
import random

import numpy as np
import pytest

from oracle import model as M
from tests import scalar_edge_cases as S
from zkp_amd import engine as EN

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in S.CATALOGUE]
K16 = sum(1 << (16 * w + 15) for w in range(16))                 # recoding constant of c = 16: carry window = 1 iff s >= 2^256 - K16


@pytest.fixture(scope="module")
def eng():
    e = EN.Engine(0, test_hooks=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def base_points():
    """64 points with known discrete logs (point 0 is B itself), their encodings as an array"""
    rng = random.Random(1234)
    logs = [rng.randrange(1, M.L) for _ in range(64)]
    logs[0] = 1
    encs = [M.ristretto_encode(M.pt_mul(k, M.BASEPOINT)) for k in logs]
    return logs, np.frombuffer(b"".join(encs), np.uint8).reshape(64, 32)


def _rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def _expected(scal, idx, logs):
    """enc((sum_i s_i k_idx(i) mod l) B) from byte-column sums per point index (exact: a column sum stays below 2^53)"""
    tot = 0
    for col in range(32):
        cs = np.bincount(idx, weights=scal[:, col].astype(np.float64), minlength=len(logs))
        tot += sum(int(x) * k for x, k in zip(cs, logs)) << (8 * col)
    return M.ristretto_encode(M.pt_mul(tot % M.L, M.BASEPOINT))


# ---- a. one scalar at a time ------------------------------------------------------------------------------------------------------------------
def test_one_catalogue_scalar_per_smallest_pippenger_call(eng, base_points):
    """n = 193, the smallest call on the Pippenger path (c = 7): term 0 is s * B, the other 192 terms are 0 * (random points).  A failure
    names the scalar."""
    logs, encs = base_points
    rng = np.random.default_rng(193)
    n = 193
    idx = rng.integers(0, 64, size=n)
    idx[0] = 0
    pts = np.ascontiguousarray(encs[idx])
    scal = np.zeros((n, 32), np.uint8)
    bad = []
    for name, s in S.CATALOGUE:
        scal[0] = _rows([s])[0]
        got = eng.msm_optional(scal, pts)
        sched = eng.last_schedule()
        assert sched["opt_pip"] == 1 and sched["pip_c"] == 7, sched
        if got != M.ristretto_encode(M.pt_mul(s % M.L, M.BASEPOINT)):
            bad.append(name)
    assert not bad, bad


# ---- b. mixed calls, one per window size ----------------------------------------------------------------------------------------------------
def _mixed_call(n, tile, logs, seed):
    """scalars [n][32], point indices: uniformly random 32-byte strings (15 in 16 are >= l), every catalogue entry at a random place, and
    catalogue entries at index 0, n - 1 and on both sides of every sort-tile boundary (the carry and fold entries first)"""
    rng = np.random.default_rng(seed)
    scal = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    idx = rng.integers(0, len(logs), size=n)
    edges = [0, n - 1] + [p for b in range(tile, n, tile) for p in (b - 1, b)]
    first = ["pip16:carry_min", "2^256-1", "pip16:carry_below", "l", "half+1", "half", "2^255"]
    order = [i for f in first for i, nm in enumerate(NAMES) if f in nm.split("=")] + list(range(len(NAMES)))
    assert len(order) >= len(NAMES) + 5
    cat = _rows(S.VALUES)
    taken = set(edges)
    for k, p in enumerate(edges):
        scal[p] = cat[order[k % len(order)]]
    free = [int(p) for p in rng.permutation(n)[:len(NAMES) + len(edges)] if int(p) not in taken][:len(NAMES)]
    assert len(free) == len(NAMES)
    scal[free] = cat
    return scal, idx


MIXED = {7: (2048, 2048), 10: (4096, 2048), 11: (8192, 2048), 16: (1 << 21, 65536)}       # c: (smallest n that selects c and holds the catalogue, sort_cfg<c>::TILE)


@pytest.fixture(scope="module")
def mixed(base_points):
    """the three small mixed calls and their expectations, shared by the host-pointer, device-pointer and merge-form tests"""
    logs, encs = base_points
    out = {}
    for c in (7, 10, 11):
        n, tile = MIXED[c]
        scal, idx = _mixed_call(n, tile, logs, 700 + c)
        out[c] = (scal, np.ascontiguousarray(encs[idx]), _expected(scal, idx, logs))
    return out


@pytest.mark.parametrize("c", [7, 10, 11])
def test_mixed_call_per_window_size(eng, mixed, c):
    scal, pts, want = mixed[c]
    got = eng.msm_optional(scal, pts)
    sched = eng.last_schedule()
    assert sched["opt_pip"] == 1 and sched["pip_c"] == c, sched
    assert got == want


@pytest.mark.parametrize("c", [7, 11])
def test_mixed_call_on_device_buffers(eng, mixed, c):
    import torch
    assert torch.cuda.is_available()
    scal, pts, want = mixed[c]
    d_sc, d_pts = torch.from_numpy(scal).to("cuda:0"), torch.from_numpy(pts).to("cuda:0")
    d_out = torch.ones(32, dtype=torch.uint8, device="cuda:0")
    d_st = torch.ones(1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng.msm_optional_dev(len(scal), d_sc.data_ptr(), d_pts.data_ptr(), d_out.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    sched = eng.last_schedule()
    assert sched["opt_pip"] == 1 and sched["pip_c"] == c, sched
    assert int(d_st.cpu()[0]) == 0 and d_out.cpu().numpy().tobytes() == want


def test_mixed_call_on_both_merge_forms(eng, mixed):
    scal, pts, want = mixed[11]
    try:
        for mode, form in ((1, 0), (2, 1)):
            eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, mode)
            got = eng.msm_optional(scal, pts)
            sched = eng.last_schedule()
            assert sched["pip_c"] == 11 and sched["pip_merge"] == form, (mode, sched)
            assert got == want, "merge mode %d" % mode
    finally:
        eng.set_option(EN.ZKP_TESTOPT_PIP_MERGE, 0)


def test_mixed_call_with_the_carry_window(eng, base_points):
    """c = 16 from 2^21 terms on: the only window size whose carry window a 256-bit scalar can reach (256 = 16 * 16, so s + K overflows bit 255
    when s >= 2^256 - K; about half of the uniformly random scalars do).  The second call has the same points and the same scalars with bit
    255 cleared -- and bit 254 too in the few that are still >= 2^256 - K = 0x7fff7fff...8000 -- so its carry window is empty: if only the
    first call is wrong, the carry window's bucket row, its slot in k_pip_combine or the start of the Horner tail is."""
    logs, encs = base_points
    n, tile = MIXED[16]
    scal, idx = _mixed_call(n, tile, logs, 716)
    pts = np.ascontiguousarray(encs[idx])
    assert sum(1 for p in [0, n - 1, tile - 1, tile] if int.from_bytes(scal[p].tobytes(), "little") >= 2**256 - K16) >= 2
    assert int((scal[:, 31] >= 0x80).sum()) > n // 4                          # every one of them has a carry digit
    plain = scal.copy()
    plain[:, 31] &= 0x7f
    for p in np.nonzero((plain[:, 31] == 0x7f) & (plain[:, 30] == 0xff))[0]:     # the only rows that can still be >= 2^256 - K
        if int.from_bytes(plain[p].tobytes(), "little") >= 2**256 - K16:
            plain[p, 31] &= 0x3f
    want, want_plain = _expected(scal, idx, logs), _expected(plain, idx, logs)
    got = eng.msm_optional(scal, pts)
    sched = eng.last_schedule()
    got_plain = eng.msm_optional(plain, pts)
    sched_plain = eng.last_schedule()
    assert sched["pip_c"] == 16 and sched_plain["pip_c"] == 16, (sched, sched_plain)
    assert got_plain == want_plain, "c = 16 without a carry digit"
    assert got == want, "c = 16 with carry digits (the call without them is right)"


# ---- c. zkp_msm_many: every catalogue entry on every class of point ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_job(base_points):
    """One job of 148-odd MSMs of 7 terms (> 1,024 terms: the classified path): three terms on registered points (fixed-base walk; crossbar
    look-ups under ZKP_CT), three on shared cold points (comb tables), one on a point no other term uses (the ladder under ZKP_VARTIME, a
    comb table walked with masked scans under ZKP_CT).  MSM m takes catalogue entries m, m + 49, m + 98 (mod N) on each of the first two
    kinds and entry m on its single-use point, so every entry meets every kind."""
    logs64, encs64 = base_points
    rng = random.Random(2025)
    N = len(S.VALUES)
    single_logs = [rng.randrange(1, M.L) for _ in range(N)]
    single = np.frombuffer(b"".join(M.ristretto_encode(M.pt_mul(k, M.BASEPOINT)) for k in single_logs), np.uint8).reshape(N, 32)
    n_reg, n_cold = 12, 8
    logs = logs64[:n_reg + n_cold] + single_logs
    points = np.concatenate([encs64[:n_reg + n_cold], single])
    off, scalars, pidx = [0], [], []
    for m in range(N):
        for k, d in enumerate((0, 49, 98)):
            scalars.append(S.VALUES[(m + d) % N]); pidx.append((m + 5 * k) % n_reg)
            scalars.append(S.VALUES[(m + d) % N]); pidx.append(n_reg + (m + 3 * k) % n_cold)
        scalars.append(S.VALUES[m]); pidx.append(n_reg + n_cold + m)
        off.append(len(scalars))
    assert len(scalars) > 1024
    want = []
    for m in range(N):
        dlog = sum(scalars[t] * logs[pidx[t]] for t in range(off[m], off[m + 1])) % M.L
        want.append(M.ristretto_encode(M.pt_mul(dlog, M.BASEPOINT)))
    return off, _rows(scalars), pidx, points, np.ascontiguousarray(encs64[:n_reg]), want


@pytest.mark.parametrize("flags", [EN.ZKP_VARTIME, EN.ZKP_CT])
def test_msm_many_catalogue_on_every_point_class(many_job, flags):
    off, scal, pidx, points, registered, want = many_job
    e = EN.Engine(0, test_hooks=True)
    try:
        e.prepare_fixed_points(registered)
        out, st = e.msm_many(off, scal, pidx, points, flags)
        sched = e.last_schedule()
    finally:
        e.close()
    assert sched["terms_split"] == 1 and sched["comb_min"] == (1 if flags == EN.ZKP_CT else 2), sched
    assert not st.any()
    bad = [m for m in range(len(want)) if out[m].tobytes() != want[m]]
    assert not bad, [(m, NAMES[m]) for m in bad[:8]]

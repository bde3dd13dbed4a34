"""The sign-folded walk of vouched scalars.  A constant-time call whose caller vouches that every scalar is reduced mod l (the fused prove
flows; ZKP_TESTOPT_VOUCH_REDUCED of the test-hook build for zkp_msm_many) skips the carry window, and its fixed-base blocks walk min(s, l - s)
in 36 windows of 7 bits -- the last one read without the offset -- and negate the result where l - s was walked (hot_tables.h).

The fused prove flow derives its blindings, so edge scalars cannot be planted there: zkp_msm_many is fed a catalogue of reduced scalars --
0, 1, (l - 1) / 2 (the largest folded value), (l + 1) / 2, l - 1, 2^251 - 1, 2^251, 2^251 + 1, the values around the first carry into
window 35, and digits +-64 and +-63 in windows 0, 34 and 35, each as s and as l - s -- on every class of point, with 1, 63, 64 and 65 terms per
class (a lane, a wavefront less one, a wavefront, a wavefront and a lane).  Expectations are exact multiples of the base point from
oracle/model.py; the same job without the vouching flag gives the same bytes.  One fused CMZ prove and one fused DLEQ prove of 65 proofs are
compared with oracle/c's prover byte for byte."""
import random

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests import degenerate_cases as D
from zkp_amd import engine as EN
from zkp_amd import toolbox as T

pytestmark = pytest.mark.gpu

L = M.L
HALF = (L - 1) // 2
W = 7                                          # HOT_W
K35 = sum(1 << (W * w + W - 1) for w in range(35))          # the offsets of windows 0 .. 34 of a folded walk
SIZES = (1, 63, 64, 65)


def _window_digit(w, d):
    """the reduced scalar whose only non-zero signed digit is d in window w, as an integer mod l"""
    return (d << (W * w)) % L


def _catalogue():
    cat = [0, 1, HALF, HALF + 1, L - 1, 2**251 - 1, 2**251, 2**251 + 1]
    cat += [HALF - 1, HALF + 2]                                               # (HALF itself is the largest value the fold leaves alone)
    # the first carry into window 35: s + K35 reaches 2^245 at s = 2^245 - K35
    cat += [2**245 - K35 - 1, 2**245 - K35, 2**245 - K35 + 1, 2**245 - 1, 2**245]
    for w in (0, 34, 35):
        for d in (64, 63, -63, -64):
            s = _window_digit(w, d)
            cat += [s, (L - s) % L]                                           # without and with the fold (whichever of the two is above HALF folds)
    out = []
    for v in cat:
        assert 0 <= v < L
        if v not in out:
            out.append(v)
    return out


CAT = _catalogue()


def test_the_catalogue_holds_what_the_walk_can_get_wrong():
    """(no GPU work) the folded value of every entry fits 36 windows with a last window of at most 64, and 64 is reached"""
    assert {0, 1, HALF, HALF + 1, L - 1, 2**251 - 1, 2**251, 2**251 + 1} <= set(CAT) and len(CAT) <= 63
    tops = set()
    for s in CAT:
        f = s if s <= HALF else L - s
        e = f + K35
        assert e >> 252 == 0
        tops.add(e >> 245)
        digits = [((e >> (W * w)) & 127) - 64 for w in range(35)] + [e >> 245]
        assert sum(d << (W * w) for w, d in enumerate(digits)) == f
    assert max(tops) == 64 and 0 in tops and 63 in tops
    assert any(s > HALF for s in CAT) and any(0 < s <= HALF for s in CAT)


def _enc(k):
    return M.ristretto_encode(M.pt_mul(k % L, M.BASEPOINT))


@pytest.fixture(scope="module")
def pool():
    """points with known discrete logs: 12 to register (4 carry the catalogue, 8 carry filler terms), 7 used 10 times each, 22 used 2 - 4 times,
    65 used once"""
    rng = random.Random(36)
    logs = [rng.randrange(1, L) for _ in range(12 + 7 + 22 + 65)]
    return logs, np.frombuffer(b"".join(_enc(k) for k in logs), np.uint8).reshape(len(logs), 32)


def _job(n, logs):
    """-> off, scalars (integers), pidx.  Classes of the term kernel under ZKP_CT with single-use points on the ladder:
      fixed-base   registered points 0 .. 3, n catalogue terms each (a class per table); registered points 4 .. 11 carry 128 filler terms each,
                   which put the call on the classified path (1,024 terms) without adding to any class below
      grouped      points used 10 times, one per MSM in consecutive MSMs: 7 of them (70 terms: across the 31-term half and the 62-term
                   wavefront of the grouped walk); one for n = 1
      comb scan    n terms on points used 3 times (n = 1: one point used twice, the smallest this class gets; a remainder joins the last point)
      ladder       n points used once
    term i of a class takes catalogue entry (i + shift) mod len(CAT): from n = 63 on every entry meets every class"""
    rng = random.Random(n)
    R, G, Cb, S = 0, 12, 19, 41
    terms = []                                                                # (scalar, point) in MSM order
    groups = 7 if n > 1 else 1
    msms = []
    for g in range(groups):                                                   # MSM g: ten terms on group point g
        msms.append([(CAT[(10 * g + i) % len(CAT)], G + g) for i in range(10)])
    for p in range(4):
        terms += [(CAT[(i + 11 * p) % len(CAT)], R + p) for i in range(n)]
    n_comb = max(n, 2)
    uses = [3] * (n_comb // 3)
    if n_comb % 3:
        if uses and n_comb % 3 == 1:
            uses[-1] += 1
        else:
            uses.append(n_comb % 3)
    assert sum(uses) == n_comb and all(2 <= u <= 4 for u in uses) and len(uses) <= 22
    i = 0
    for q, u in enumerate(uses):
        for _ in range(u):
            terms.append((CAT[(i + 5) % len(CAT)], Cb + q))
            i += 1
    terms += [(CAT[(i + 23) % len(CAT)], S + i) for i in range(n)]
    for p in range(4, 12):
        terms += [(rng.randrange(L), R + p) for _ in range(128)]
    rng.shuffle(terms)
    for k in range(0, len(terms), 9):
        msms.append(terms[k:k + 9])
    off, scal, pidx = [0], [], []
    for m in msms:
        scal += [s for s, _ in m]
        pidx += [p for _, p in m]
        off.append(len(scal))
    assert len(scal) >= 1024
    want = [_enc(sum(s * logs[p] for s, p in m)) for m in msms]
    return np.array(off, np.uint32), scal, np.array(pidx, np.uint32), want


def _rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


@pytest.fixture(scope="module")
def jobs(pool):
    logs, _ = pool
    return {n: _job(n, logs) for n in SIZES}


@pytest.fixture(scope="module")
def eng(pool):
    _, encs = pool
    e = EN.Engine(0, test_hooks=True)
    e.prepare_fixed_points(np.ascontiguousarray(encs[:12]))
    e.set_option(EN.ZKP_OPT_CT_SINGLE_USE_TABLES, 0)                           # single-use points: the constant-time ladder
    e.set_option(EN.ZKP_OPT_GROUPED_COMB, 1)                                   # points with ten uses: the grouped walk, whatever the call's size
    yield e
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_vouched_catalogue_on_every_class(eng, pool, jobs, n):
    _, encs = pool
    off, scal, pidx, want = jobs[n]
    rows = _rows(scal)
    outs = {}
    try:
        for vouch in (1, 0):
            eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, vouch)
            out, st = eng.msm_many(off, rows, pidx, encs, EN.ZKP_CT)
            sched = eng.last_schedule()
            assert sched.get("terms_split") == 1 and sched.get("grouped") == 1 and sched.get("comb_min") == 2, sched
            assert sched.get("no_carry") == vouch and sched.get("sign_fold") == vouch, sched
            assert not st.any()
            outs[vouch] = out
    finally:
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, 0)
    bad = [m for m in range(len(want)) if outs[1][m].tobytes() != want[m]]
    assert not bad, ("vouched", bad[:8])
    assert (outs[0] == outs[1]).all()                                          # the same job without the flag: the same bytes


def test_variable_time_calls_never_fold(eng, pool, jobs):
    _, encs = pool
    off, scal, pidx, want = jobs[64]
    try:
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, 1)
        out, st = eng.msm_many(off, _rows(scal), pidx, encs, EN.ZKP_VARTIME)
        sched = eng.last_schedule()
    finally:
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, 0)
    assert sched.get("no_carry") == 0 and sched.get("sign_fold") == 0, sched
    assert not st.any() and [o.tobytes() for o in out] == want


def _fused_prove(stname, statement, label, n, seed):
    """one fused prove of n ordinary proofs on the test-hook build -> (batch, entropy, challenges, responses, commitments, schedule)"""
    import torch
    assert torch.cuda.is_available(), "torch cannot see the GPU in this process"
    b = D.build_batch(stname, n, {}, seed)
    m, nc = len(b.shape.secret_names), len(b.shape.cons)
    entropy = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    e = EN.Engine(0, test_hooks=True)
    try:
        fst = EN.FusedStatement(b.shape.label, *statement)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
        t0 = T.Transcript(label).state
        pos = int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16
        e.prepare_fixed_points(b.common)
        d_tbl = dev(np.concatenate([b.common, b.inst.reshape(-1, 32)]))
        d_ts, d_sec, d_ent = dev(np.stack([t0] * n)), dev(b.secrets), dev(entropy)
        d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, m, 32), z(n, nc, 32), z(nc * n)
        torch.cuda.synchronize()
        e.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                          d_coms.data_ptr(), d_st.data_ptr())
        e.synchronize()
        sched = e.last_schedule()
        assert not d_st.cpu().numpy().any()
        return b, entropy, d_chal.cpu().numpy(), d_resp.cpu().numpy(), d_coms.cpu().numpy(), sched
    finally:
        e.close()


@pytest.mark.parametrize("stname", ["cmz10", "dleq_macro"])
def test_fused_prove_of_65_proofs_equals_the_c_oracle(stname):
    import bench
    statement = bench.cmz_statement() if stname == "cmz10" else bench.dleq_macro_statement()
    n = 65
    b, entropy, chal, resp, coms, sched = _fused_prove(stname, statement, b"sign-fold", n, 6500 + len(stname))
    if stname == "cmz10":                                                      # 2,015 terms: the classified path (DLEQ's 130 terms take a lane each)
        assert sched.get("terms_split") == 1 and sched.get("no_carry") == 1 and sched.get("sign_fold") == 1, sched
    _, cst = b.shape.build()
    for j in range(n):
        ec, er, ek, _ = C.prove(cst, b"sign-fold", b.secrets[j], D.points_of(b, j), entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), "proof %d differs from the oracle's" % j

"""The comb walks and the ladder of a constant-time call that vouches for reduced scalars (the fused prove flows; ZKP_TESTOPT_VOUCH_REDUCED of the
test-hook build for zkp_msm_many): the grouped walk in Horner order (12 doublings), tables without the carry tooth, and the sign fold in the
radix-16 walks -- min(s, l - s) recoded with the offset on nibbles 0 .. 61 only, nibble 62 read as it stands, the sum negated where l - s was
walked (sc25519.h: sc_fold_recode16; comb_tables.h: comb_group_xbar, term_comb, term_ladder16).

The fused prove flow derives its blindings, so edge scalars cannot be planted there: zkp_msm_many is fed the catalogue of
tests/comb_fold_cases.py on the grouped class (7 points x 10 uses: across the 31-term half and the 62-term wavefront), the comb-scan class and the
ladder class, with 1, 63, 64 and 65 terms per class.  Expectations are exact multiples of the base point from oracle/model.py; the same job
without the vouching flag gives the same bytes.  A vouched call leaves the carry entry of its tables unwritten: on a workspace filled with
0xFFFFFFFF a vouched call is followed, without a refill, by an unvouched one whose scalars need that entry.  Single-use points with
ZKP_OPT_CT_SINGLE_USE_TABLES = 1 drive the 4-teeth tables and scans, through the quad builder and the one-lane builder.  Fused CMZ proves of 65
proofs (Q on the folded constant-time ladder) and of 1 proof (31 terms: one lane per term, no classes) are compared with oracle/c's prover byte
for byte."""
import random

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests import comb_fold_cases as F
from tests import degenerate_cases as D
from zkp_amd import engine as EN
from zkp_amd import toolbox as T

L = M.L
CAT = F.CAT
SIZES = (1, 63, 64, 65)
N_REG, N_GROUP, N_COMB, N_SINGLE = 8, 7, 22, 65
CARRY_SCALARS = (2**256 - 1, 2**255 + 2**251, 2**256 - 2**4)       # 65 radix-16 digits each: they need the carry entry 2^256 P


def test_the_catalogue_reaches_top_digits_0_and_8():
    """(no GPU work) and over the three multi-term sizes every entry meets every class"""
    tops = set()
    for s in CAT:
        f, _ = F.fold(s)
        d = F.digits(f)
        assert all(-8 <= x <= 7 for x in d[:-1]) and sum(x << (4 * i) for i, x in enumerate(d)) == f
        tops.add(d[-1])
    assert 0 in tops and 8 in tops and max(tops) == 8
    assert any(F.fold(s)[1] for s in CAT) and any(not F.fold(s)[1] and s for s in CAT)
    for cls in range(3):
        seen = set()
        for n in SIZES[1:]:
            seen |= {(i + _shift(n, cls)) % len(CAT) for i in range(70 if cls == 0 else n)}
        assert len(seen) == len(CAT), cls
    for s in CARRY_SCALARS:
        assert (s + int("8" * 64, 16)) >> 256 == 1


def _shift(n, cls):
    return 29 * SIZES.index(n) + 11 * cls


def _enc(k):
    return M.ristretto_encode(M.pt_mul(k % L, M.BASEPOINT))


@pytest.fixture(scope="module")
def pool():
    """points with known discrete logs: 8 to register (they carry filler terms), 7 used 10 times each, 22 used 2 - 4 times, 65 used once"""
    rng = random.Random(62)
    logs = [rng.randrange(1, L) for _ in range(N_REG + N_GROUP + N_COMB + N_SINGLE)]
    return logs, np.frombuffer(b"".join(_enc(k) for k in logs), np.uint8).reshape(len(logs), 32)


def _job(n, logs, scalar_of):
    """-> off, scalars (integers), pidx, expected encodings.  Classes of the term kernel under ZKP_CT with single-use points on the ladder:
      grouped      points used 10 times, one per MSM in consecutive MSMs: 7 of them (70 terms); one for n = 1
      comb scan    n terms on points used 3 times (n = 1: one point used twice; a remainder joins the last point)
      ladder       n points used once
      fixed-base   registered points 0 .. 7 carry 128 filler terms each, which put the call on the classified path (1,024 terms)
    term i of class cls takes scalar_of(i + shift(n, cls))"""
    rng = random.Random(n)
    G, Cb, S = N_REG, N_REG + N_GROUP, N_REG + N_GROUP + N_COMB
    groups = N_GROUP if n > 1 else 1
    msms = [[(scalar_of(10 * g + i + _shift(n, 0)), G + g) for i in range(10)] for g in range(groups)]
    terms = []
    n_comb = max(n, 2)
    uses = [3] * (n_comb // 3)
    if n_comb % 3:
        if uses and n_comb % 3 == 1:
            uses[-1] += 1
        else:
            uses.append(n_comb % 3)
    assert sum(uses) == n_comb and all(2 <= u <= 4 for u in uses) and len(uses) <= N_COMB
    i = 0
    for q, u in enumerate(uses):
        for _ in range(u):
            terms.append((scalar_of(i + _shift(n, 1)), Cb + q))
            i += 1
    terms += [(scalar_of(i + _shift(n, 2)), S + i) for i in range(n)]
    for p in range(N_REG):
        terms += [(rng.randrange(L), p) for _ in range(128)]
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
    return {n: _job(n, logs, lambda i: CAT[i % len(CAT)]) for n in SIZES}


@pytest.fixture(scope="module")
def eng(pool):
    _, encs = pool
    e = EN.Engine(0, test_hooks=True)
    e.prepare_fixed_points(np.ascontiguousarray(encs[:N_REG]))
    e.set_option(EN.ZKP_OPT_CT_SINGLE_USE_TABLES, 0)                           # single-use points: the constant-time ladder
    e.set_option(EN.ZKP_OPT_GROUPED_COMB, 1)                                   # points with ten uses: the grouped walk, whatever the call's size
    yield e
    e.close()


def _call(eng, encs, job, vouch):
    off, scal, pidx, _ = job
    try:
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, vouch)
        out, st = eng.msm_many(off, _rows(scal), pidx, encs, EN.ZKP_CT)
        sched = eng.last_schedule()
    finally:
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, 0)
    assert sched.get("terms_split") == 1 and sched.get("grouped") == 1 and sched.get("comb_min") == 2, sched
    assert sched.get("no_carry") == vouch and sched.get("sign_fold") == vouch, sched
    assert not st.any()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_vouched_catalogue_on_the_grouped_scan_and_ladder_classes(eng, pool, jobs, n):
    _, encs = pool
    want = jobs[n][3]
    outs = {vouch: _call(eng, encs, jobs[n], vouch) for vouch in (1, 0)}
    bad = [m for m in range(len(want)) if outs[1][m].tobytes() != want[m]]
    assert not bad, ("vouched", bad[:8])
    assert (outs[0] == outs[1]).all()                                          # the same job without the flag: the same bytes


@pytest.mark.gpu
def test_an_unvouched_call_after_a_vouched_one_builds_its_own_carry_tooth(eng, pool, jobs):
    """every word of the workspace is 0xFFFFFFFF, the vouched call leaves entry 128 of its tables at that, and the unvouched call on the same
    points -- same table slots -- must write the entry before its walks add it"""
    logs, encs = pool
    eng.debug_fill_workspace(1 << 26, 0xFFFFFFFF)
    ws = eng.debug_ws_bytes()
    out = _call(eng, encs, jobs[65], 1)
    assert [o.tobytes() for o in out] == jobs[65][3]
    carry = _job(65, logs, lambda i: CARRY_SCALARS[i % 3])
    out = _call(eng, encs, carry, 0)
    assert eng.debug_ws_bytes() == ws, "a call grew the workspace after the fill: it saw fresh memory"
    bad = [m for m in range(len(carry[3])) if out[m].tobytes() != carry[3][m]]
    assert not bad, ("unvouched after vouched", bad[:8])


def _single_use_job(n, logs):
    """n cold points used once each and one used twice (catalogue scalars) + the fixed-base filler: with ZKP_OPT_CT_SINGLE_USE_TABLES = 1 and a shared
    cold point in the job every cold point gets a comb table, and with fewer than two terms per table on average the host entry builds 4-TEETH tables
    (pick_teeth; comb_tables.h: a 33-entry table, 16 windows per tooth -- nibble 63 is tooth 3's window 15, nibble 62 its window 14)"""
    rng = random.Random(400 + n)
    S = N_REG + N_GROUP + N_COMB
    terms = [(CAT[(i + 7) % len(CAT)], S + i) for i in range(n)]
    terms += [(CAT[3], N_REG + N_GROUP), (CAT[4], N_REG + N_GROUP)]            # the shared cold point: without one, single-use points walk the ladder
    for p in range(N_REG):
        terms += [(rng.randrange(L), p) for _ in range(128)]
    rng.shuffle(terms)
    msms = [terms[k:k + 9] for k in range(0, len(terms), 9)]
    off, scal, pidx = [0], [], []
    for m in msms:
        scal += [s for s, _ in m]
        pidx += [p for _, p in m]
        off.append(len(scal))
    want = [_enc(sum(s * logs[p] for s, p in m)) for m in msms]
    return np.array(off, np.uint32), scal, np.array(pidx, np.uint32), want


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [0, 1], ids=["quad_builder", "lane_builder"])
def test_vouched_four_teeth_tables_and_their_scans(eng, pool, lane):
    """term_comb<true, 4> folded, on tables without the carry tooth from k_comb_tables<4> and from k_comb_tables_lane_nc<4>; the same bytes unvouched"""
    logs, encs = pool
    off, scal, pidx, want = _single_use_job(N_SINGLE, logs)
    outs, tables = {}, {}
    try:
        eng.set_option(EN.ZKP_OPT_CT_SINGLE_USE_TABLES, 1)
        eng.set_option(EN.ZKP_OPT_TABLES_LANE, lane)
        eng.set_profiling(True)
        for vouch in (1, 0):
            eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, vouch)
            out, st = eng.msm_many(off, _rows(scal), pidx, encs, EN.ZKP_CT)
            sched = eng.last_schedule()
            assert sched.get("terms_split") == 1 and sched.get("comb_min") == 1, sched
            assert sched.get("no_carry") == vouch and sched.get("sign_fold") == vouch, sched
            assert not st.any()
            outs[vouch], tables[vouch] = out, eng.last_kernels().get("tables", [])
    finally:
        eng.set_profiling(False)
        eng.set_option(EN.ZKP_TESTOPT_VOUCH_REDUCED, 0)
        eng.set_option(EN.ZKP_OPT_TABLES_LANE, 2**64 - 1)
        eng.set_option(EN.ZKP_OPT_CT_SINGLE_USE_TABLES, 0)
    print("tables kernels:", tables)
    assert tables[1] == ["zkp::k_comb_tables_lane_nc<4>" if lane else "zkp::k_comb_tables<4>"], tables
    assert tables[0] == ["zkp::k_comb_tables_lane<4>" if lane else "zkp::k_comb_tables<4>"], tables
    bad = [m for m in range(len(want)) if outs[1][m].tobytes() != want[m]]
    assert not bad, ("vouched", bad[:8])
    assert (outs[0] == outs[1]).all()


def _fused_prove(statement, label, n, seed):
    """one fused CMZ prove of n ordinary proofs on the test-hook build, Q on the constant-time ladder -> (batch, entropy, challenges, responses,
    commitments, schedule)"""
    import torch
    assert torch.cuda.is_available(), "torch cannot see the GPU in this process"
    b = D.build_batch("cmz10", n, {}, seed)
    m, nc = len(b.shape.secret_names), len(b.shape.cons)
    entropy = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    e = EN.Engine(0, test_hooks=True)
    try:
        e.set_option(EN.ZKP_OPT_CT_SINGLE_USE_TABLES, 0)
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


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1])
def test_fused_cmz_prove_with_q_on_the_ladder_equals_the_c_oracle(n):
    import bench
    b, entropy, chal, resp, coms, sched = _fused_prove(bench.cmz_statement(), b"comb-fold", n, 6200 + n)
    if n == 65:                                                                # 2,015 terms: the classified path, Q on the folded ladder
        assert sched.get("terms_split") == 1 and sched.get("no_carry") == 1 and sched.get("sign_fold") == 1, sched
    else:                                                                      # 31 terms take a lane each (k_terms_r4): no classes, no ladder, nothing vouched
        assert sched.get("terms_split") == 0 and "no_carry" not in sched and "sign_fold" not in sched, sched
    _, cst = b.shape.build()
    for j in range(n):
        ec, er, ek, _ = C.prove(cst, b"comb-fold", b.secrets[j], D.points_of(b, j), entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), "proof %d differs from the oracle's" % j

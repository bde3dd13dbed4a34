"""A reused context gives the bytes of a fresh one: every workspace layout behind a workspace that earlier calls have written all over.

The device workspace of a context only grows and is never cleared, and a server keeps one context for days.  A fresh hipMalloc is zero in
practice, and 0 reads as "accepted", "no decode failure", "count 0": a kernel that reads a word before this call wrote it passes every
test that runs on a fresh context.  Here zkp_debug_fill_workspace (test-hook build) sets EVERY word of the workspace to 0 (the control:
what a fresh allocation holds), 3 (both bits of the two-bit status words, a small nonzero counter or cursor) or 0xFFFFFFFF in front of
each call, and the call must still give

* what an independent reference says: exact discrete logs and the C oracle for the MSMs, the C oracle's prover byte for byte for the
  proofs, exactly the planted mutants for the verdicts (every other proof accepted: the 0xFFFFFFFF direction; every mutant rejected:
  the 0 direction), Python integers / hashlib / the host backend for the rest;
* the bytes of a FRESH context of the shipped library;
* on the path the case is meant for (zkp_debug_last_schedule, the keys of tests/size_thresholds.py).

The shapes are the smallest that reach each layout ("Workspace regions and their first writers").  The fill is sized so that
no case grows the workspace after it -- a call that had to reallocate would see fresh memory again -- and zkp_debug_ws_bytes is compared
after every call with its value right after the fill.

Entry point that calls ensure_ws (include/zkp_mi355x.h sections 1 to 14) -> the test that fills the workspace in front of it.  "here" is this
module; the other files hold a test_results_do_not_depend_on_what_the_workspace_held of their own.

  zkp_msm_many                                                    here: test_msm_many
  zkp_msm_optional, zkp_msm_optional_dev (msm_optional_impl)      here: test_msm_optional (the host-pointer form; _dev carves through the same function)
  zkp_decode_check, zkp_encode_many                               here: test_decode_check_and_encode_many
  zkp_fused_prove_dev                                             here: test_prove
  zkp_fused_verify_compact_dev, zkp_fused_verify_batchable_dev    here: test_verify
  zkp_fused_batch_verify_dev, zkp_fused_batch_verify_many_dev     here: test_batch_verify_one_batch, test_batch_verify_three_batches
  zkp_batch_check                                                 here: test_batch_check (the raw call on the test-hook context)
  the host-buffer jobs (prove_job, verify_compact_job,            here: test_ragged (the _ragged calls are these jobs over class programs)
    verify_batchable_job, batch_verify_job)
  zkp_fused_hash_to_group_ragged                                  here: test_ragged[hash]
  zkp_fused_hash_to_group (aligned)                               here: test_aligned_hash_to_group
  zkp_from_uniform_bytes, zkp_hash_from_bytes_sha512,             here: test_other_calls
    zkp_sc_hash_from_bytes_sha512 (hash_from_bytes_host),
    zkp_sc_random
  zkp_sc_invert, zkp_sc_from_wide, zkp_sc_muladd                  here: test_scalar_calls (every stride combination at n = 257)
  zkp_transcripts_append_message, _challenge_bytes,               here: test_transcript_calls
    _witness_rng, _challenge_scalars, _append_points
  zkp_mul_base, zkp_mul_points                                    tests/test_gpu_point_mul.py
  zkp_add_points, zkp_sum_points                                  tests/test_gpu_point_sum.py
  zkp_msm_segments                                                tests/test_gpu_msm_segments.py
  zkp_msm_segments_dev                                            here: test_msm_segments_dev (the generic-bounds terms_cfg, not host_terms_cfg, and an index
                                                                  k_iota writes into the workspace); tests/test_gpu_msm_segments.py fills in front of it too
  zkp_msm_optional_many                                           tests/test_gpu_msm_optional_many.py, tests/test_gpu_msm_optional_many_edges.py
  zkp_msm_optional_many_dev                                       tests/test_gpu_msm_optional_many_edges.py: test_results_do_not_depend_on_what_the_workspace_held
                                                                  (one class padded to max_seg, and the term path under generic bounds up to max_seg = S: neither
                                                                  is the plan of its host-pointer form)
  zkp_sc_reduce                                                   tests/test_gpu_scalar_reduce.py
  zkp_sc_scan, zkp_scan_points                                    tests/test_gpu_scan.py
  zkp_dlog_base                                                   tests/test_gpu_dlog.py
  zkp_dlog_point                                                  tests/test_gpu_dlog_point.py
  zkp_mul_points_dev, zkp_sum_points_dev, zkp_sc_reduce_dev,      not filled directly: each carves the layout of its host-pointer form (above) less
    zkp_sc_scan_dev, zkp_scan_points_dev, zkp_dlog_base_dev,      the staging of the operands, which the caller owns, and launches through the same
    zkp_dlog_point_dev, zkp_msm_many_dev, zkp_sc_random_dev,      launcher; those files fill the workspace in front of the host-pointer form only
    zkp_hash_from_bytes_sha512_dev                                (zkp_msm_many_dev: test_msm_many[outputs2048_dev] here does run the _dev form)
  zkp_debug_quad_selftest, zkp_debug_row_selftest                 test-hook probes: every word they read they uploaded in the same call
  carve nothing (not tested): the _dev forms of section 7 (zkp_transcripts_*_dev) and of zkp_sc_invert / _from_wide / _muladd /
    _sc_hash_from_bytes_sha512, zkp_from_uniform_bytes_dev, zkp_mul_base_dev, zkp_add_points_dev; zkp_ctx_prepare_fixed_points,
    zkp_ctx_prepare_dlog and zkp_ctx_prepare_dlog_point build into allocations of their own

The transcript calls are checked against oracle.model's Merlin in Python started from the blob (tests/product_history_cases.py), the scalar
calls against Python integers."""
import hashlib

import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from tests import product_history_cases as PH
from tests import test_gpu_thresholds as TH
from tests.test_host_scalar_ops import chacha_block, ints, want_hash

pytestmark = pytest.mark.gpu
WORDS = (0, 3, 0xFFFFFFFF)
CAP = 1 << 29                      # 512 MiB: many times what the largest ordinary case carves (8,192 constant-time terms: 45 MB)
BIG_CAP = 3 << 29                  # the 2^21-term Pippenger call carves 1.2 GB (pip_ws<16> + its two input arrays)
JUNK = np.frombuffer(bytes([1] + [0] * 31), np.uint8)          # s = 1: not a valid ristretto255 encoding
ZKP_CT, ZKP_VARTIME = 1, 0
OPT_DEV_OVERLAP = 5
IDENTITY = bytes(32)


@pytest.fixture(scope="module")
def engines():
    """(test-hook engine: the one context every case reuses; shipped engine: set-up only -- points, honest proofs)"""
    from zkp_amd.engine import Engine
    eh, es = Engine(0, test_hooks=True), Engine(0)
    yield eh, es
    eh.close()
    es.close()


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(engines):
    """a call that faulted leaves its context in error: the session ends there instead of launching the remaining cases on that card"""
    yield
    try:
        engines[0].synchronize()
    except Exception as e:                                   # noqa: BLE001 -- whatever the runtime reports
        pytest.exit("the reused context reports a GPU error; nothing further is started: %s" % e, returncode=3)
    _same_workspace(engines[0])


_WS = {"bytes": None}


def _same_workspace(eh):
    """no call since the last fill made the workspace grow: a call that reallocates sees fresh memory again and tests nothing"""
    if _WS["bytes"] is not None:
        assert eh.debug_ws_bytes() == _WS["bytes"], "a call grew the workspace after the fill (%d -> %d bytes): raise CAP" % (_WS["bytes"], eh.debug_ws_bytes())


def _fill(eh, min_bytes, word):
    """every word of a workspace of at least min_bytes = word; the size it then has is what every call up to the next fill must leave it at"""
    _same_workspace(eh)
    eh.debug_fill_workspace(min_bytes, word)
    _WS["bytes"] = eh.debug_ws_bytes()
    assert _WS["bytes"] >= min_bytes


def _fresh(schedule=None):
    """a fresh context of the shipped library (its workspace is what hipMalloc hands out)"""
    from zkp_amd.engine import Engine
    e = Engine(0)
    if schedule == "latency":
        e.set_option(OPT_DEV_OVERLAP, 2)
    return e


_REF = {}


def _once(key, make):
    """references and inputs are computed once per case and shared by its three fills"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _neg(s_row):
    return np.frombuffer(((M.L - int.from_bytes(s_row.tobytes(), "little")) % M.L).to_bytes(32, "little"), np.uint8)


# ---- msm_many ---------------------------------------------------------------------------------------------------------------------------
def _msm_job(size, unit, rng):
    """A CSR job of MSM lengths 1, 2, 3, 11 (in turn) with an empty range, two cancelling MSMs and one undecodable point; `size` counts
    terms or outputs.  3 of 4 terms lie on 64 shared points, every 4th on a point of its own (both table classes of a constant-time call).
    -> (off, scalars, pidx, n_points, junk index, identity outputs, flagged outputs)"""
    lens, total = [], 0
    cycle = (1, 2, 3, 11)
    while (total < size) if unit == "terms" else (len(lens) < size):
        k = 0 if len(lens) == 5 else (2 if len(lens) in (7, 9) else cycle[len(lens) % 4])
        if unit == "terms":
            k = min(k, size - total)
        lens.append(k)
        total += k
    assert lens[5] == 0 and lens[7] == 2 and lens[9] == 2
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n_terms = int(off[-1])
    pidx = rng.integers(0, 64, size=n_terms).astype(np.uint32)
    single = np.arange(0, n_terms, 4)
    pidx[single] = 64 + np.arange(len(single), dtype=np.uint32)
    sc = TH._rand_scalars(rng, n_terms)
    cancel = [7, 9]
    for p in cancel:                                         # s * P + (l - s) * P
        t = int(off[p])
        pidx[t + 1] = pidx[t]
        sc[t + 1] = _neg(sc[t])
    junk = 64 + len(single)                                  # one more point, undecodable, named by a term of MSM 2 (3 terms) and of the last 11-term MSM
    n_points = junk + 1
    eleven = [i for i, k in enumerate(lens) if k == 11]
    flagged = sorted({2, eleven[-1]})
    for i in flagged:
        pidx[int(off[i]) + 1] = junk
    return off, sc, pidx, n_points, junk, cancel, flagged


MSM_CASES = [  # (name, size, unit, device entry, schedule key expectations)
    ("terms1023", 1023, "terms", False, {"terms_split": 0}),
    ("terms1024", 1024, "terms", False, {"terms_split": 1, "batch_encode": 0}),
    ("terms8192", 8192, "terms", False, {"terms_split": 1}),               # constant time: quad-split scans + grouped walk (below)
    ("outputs2048_dev", 2048, "outputs", True, {"terms_split": 1, "batch_encode": 1}),
]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("flags", (ZKP_CT, ZKP_VARTIME), ids=("ct", "vartime"))
@pytest.mark.parametrize("case", MSM_CASES, ids=lambda c: c[0])
def test_msm_many(engines, case, flags, word):
    eh, es = engines
    name, size, unit, dev, expect = case

    def make():
        rng = np.random.default_rng(size + flags)
        off, sc, pidx, n_points, junk, cancel, flagged = _msm_job(size, unit, rng)
        pts, logs = TH._points(es, n_points)
        pts = pts.copy()
        pts[junk] = JUNK
        want, want_st = C.msm_many(off, sc, pidx, pts, 1 if flags == ZKP_CT else 0)           # the C oracle: every output
        assert np.flatnonzero(want_st).tolist() == flagged and not want[flagged].any()
        assert not want[cancel].any() and not want[5].any()                                    # identity outputs (two cancelling MSMs, the empty range)
        # ... and the discrete logs: the sum of the outputs that are not flagged
        keep = np.ones(len(sc), bool)
        for i in flagged:
            keep[int(off[i]):int(off[i + 1])] = False
        ones = np.zeros((len(want), 32), np.uint8)
        ones[:, 0] = 1
        assert C.msm_optional(ones, want) == TH._expected_point(TH._total_log(sc[keep], pidx[keep], logs[:junk] + [0]))
        ef = _fresh()
        try:
            fresh = TH._run_msm(ef, dev, off, sc, pidx, pts, flags)
        finally:
            ef.close()
        return off, sc, pidx, pts, want, want_st, fresh

    off, sc, pidx, pts, want, want_st, fresh = _once(("msm", name, flags), make)
    _fill(eh, CAP, word)
    out, st = TH._run_msm(eh, dev, off, sc, pidx, pts, flags)
    sched = eh.last_schedule()
    for k, v in expect.items():
        assert sched.get(k) == v, sched
    if size == 8192:
        assert sched.get("lat_split") == (1 if flags == ZKP_CT else 0) and sched.get("grouped") == (1 if flags == ZKP_CT else 0), sched
    assert (st == want_st).all(), np.flatnonzero(st != want_st)[:8]
    assert (out == want).all(), np.flatnonzero((out != want).any(axis=1))[:8]
    assert (out == fresh[0]).all() and (st == fresh[1]).all(), "a fresh context computes other bytes"


# ---- msm_optional ----------------------------------------------------------------------------------------------------------------------
OPT_CASES = [  # (name, terms, kind, schedule expectations, fills)
    ("n192", 192, "plain", {"opt_pip": 0}, WORDS),
    ("n193", 193, "plain", {"opt_pip": 1, "pip_c": 7, "pip_part": 16}, WORDS),
    ("n4096", 4096, "plain", {"opt_pip": 1, "pip_c": 10}, WORDS),
    ("n8192", 8192, "plain", {"opt_pip": 1, "pip_c": 11}, WORDS),
    ("n193_bad_point", 193, "bad", {"opt_pip": 1, "pip_c": 7}, WORDS),
    ("n193_identity", 193, "identity", {"opt_pip": 1, "pip_c": 7}, WORDS),
    ("n2097152", 1 << 21, "plain", {"opt_pip": 1, "pip_c": 16, "pip_part": 64}, (0xFFFFFFFF,)),
]
OPT_PARAMS = [(c, w) for c in OPT_CASES for w in c[4]]


@pytest.mark.parametrize("case,word", OPT_PARAMS, ids=["%s-fill%x" % (c[0], w) for c, w in OPT_PARAMS])
def test_msm_optional(engines, case, word):
    eh, es = engines
    name, n, kind, expect, _ = case

    def make():
        rng = np.random.default_rng(n + len(kind))
        pts, logs = TH._points(es, 1024)
        pidx = rng.integers(0, 1024, size=n).astype(np.uint32)
        sc = TH._rand_scalars(rng, n)
        if kind == "identity":                               # 96 cancelling pairs and a zero scalar
            for t in range(0, n - 1, 2):
                pidx[t + 1] = pidx[t]
                sc[t + 1] = _neg(sc[t])
            sc[n - 1] = 0
        big = pts[pidx]
        if kind == "bad":
            big[n // 2] = JUNK
            want = None
        else:
            want = TH._expected_point(TH._total_log(sc, pidx, logs))
            if kind == "identity":
                assert want == IDENTITY
        ef = _fresh()
        try:
            fresh = ef.msm_optional(sc, big)
        finally:
            ef.close()
        return sc, big, want, fresh

    sc, big, want, fresh = _once(("opt", name), make)
    _fill(eh, BIG_CAP if n == 1 << 21 else CAP, word)
    got = eh.msm_optional(sc, big)
    sched = eh.last_schedule()
    for k, v in expect.items():
        assert sched.get(k) == v, sched
    assert got == want
    assert got == fresh, "a fresh context computes another point"


def _torch():
    return TH._torch()


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- msm_segments_dev: the generic bounds of arrays the host has not inspected, and an index the device writes itself ------------------------
SEGMENTS_DEV_LENS = [0, 1, 600, 33, 0, 466]       # 1,100 terms: the host-pointer form would count the uses (host_terms_cfg, from 1,024 terms on); the _dev form cannot


def _segments_dev(eng, off, sc, pidx, points, flags):
    """zkp_msm_segments_dev on torch buffers, the outputs poisoned beforehand -> (out, status)"""
    torch = _torch()
    n_msm, n_terms = len(off) - 1, int(off[-1])
    d_off, d_sc, d_pts = _dev(off.view(np.int32)), _dev(sc), _dev(points)
    d_pidx = None if pidx is None else _dev(pidx.view(np.int32))
    d_out = torch.full((n_msm, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n_msm,), 0xAB, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.msm_segments_dev(n_msm, d_off.data_ptr(), d_sc.data_ptr(), None if d_pidx is None else d_pidx.data_ptr(), d_pts.data_ptr(), len(points), n_terms, flags,
                         d_out.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("own_rows", (False, True), ids=("pidx", "own_rows"))
@pytest.mark.parametrize("flags", (ZKP_CT, ZKP_VARTIME), ids=("ct", "vartime"))
def test_msm_segments_dev(engines, flags, own_rows, word):
    """1,100 terms over the 64 shared points of tests/msm_segments_cases.py, through d_pidx and with a row per term (d_pidx = NULL: k_iota writes the
    index into the workspace in front of the fold's regions)"""
    from tests import msm_segments_cases as MC
    eh, _ = engines

    def make():
        off, sc, pidx, pts = MC.job(SEGMENTS_DEV_LENS, seed=1100)
        assert int(off[-1]) >= 1024
        want, want_st = MC.expected("residue-segments-dev", off, sc, pidx, pts, flags)
        assert not want_st.any() and not want[[0, 4]].any() and want[[2, 3, 5]].any(axis=1).all()
        if own_rows:
            pidx, pts = None, np.ascontiguousarray(pts[pidx])
        ef = _fresh()
        try:
            fresh = _segments_dev(ef, off, sc, pidx, pts, flags)
        finally:
            ef.close()
        return off, sc, pidx, pts, want, want_st, fresh

    off, sc, pidx, pts, want, want_st, fresh = _once(("segments_dev", flags, own_rows), make)
    _fill(eh, CAP, word)
    out, st = _segments_dev(eh, off, sc, pidx, pts, flags)
    sched = eh.last_schedule()
    assert sched.get("terms_split") == 1 and sched.get("batch_encode") == 0, sched      # the classified term path, the fold behind it
    assert (st == want_st).all(), np.flatnonzero(st != want_st)
    assert (out == want).all(), np.flatnonzero((out != want).any(axis=1))
    assert (out == fresh[0]).all() and (st == fresh[1]).all(), "a fresh context computes other bytes"


# ---- the fused flows ------------------------------------------------------------------------------------------------------------------


def _prove_dev(eng, fst, n, ts0, pos, secrets, table, entropy, m, nc):
    """-> (challenges, responses, commitments, transcripts left behind)"""
    torch = _torch()
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
    d_ts, d_sec, d_tbl, d_ent = _dev(ts0), _dev(secrets), _dev(table), _dev(entropy)
    d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, m, 32), z(n, nc, 32), torch.full((nc * n,), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                        d_coms.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    assert not d_st.cpu().numpy().any()
    return d_chal.cpu().numpy(), d_resp.cpu().numpy(), d_coms.cpu().numpy(), d_ts.cpu().numpy()


def _batch(es, which, n):
    """n honest proofs of a statement (shipped engine, its own context), shared by the cases that verify them"""
    def make():
        fst, cst, secrets, inst, common, m, nc = TH._flow_batch(es, which, n)
        ts0, pos = TH._transcripts(n)
        entropy = np.random.default_rng(n + 2).integers(0, 256, size=(n, 32), dtype=np.uint8)
        table = np.concatenate([common, inst.reshape(-1, 32)])
        chal, resp, coms, _ = _prove_dev(es, fst, n, ts0, pos, secrets, table, entropy, m, nc)
        return dict(fst=fst, cst=cst, secrets=secrets, inst=inst, common=common, m=m, nc=nc, ts0=ts0, pos=pos, entropy=entropy, table=table,
                    chal=chal, resp=resp, coms=coms)
    return _once(("batch", which, n), make)


PROVE_CASES = [("dleq", 1, "throughput", {"terms_split": 0}), ("dleq", 65, "throughput", {"terms_split": 0}),
               ("cmz", 264, "latency", {"terms_split": 1, "lat_split": 0, "no_carry": 1}), ("cmz", 265, "latency", {"terms_split": 1, "lat_split": 1, "no_carry": 1})]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("case", PROVE_CASES, ids=lambda c: "%s-%d" % c[:2])
def test_prove(engines, case, word):
    eh, es = engines
    which, n, schedule, expect = case
    b = _batch(es, which, n)

    def make():
        ef = _fresh(schedule)
        try:
            fresh = _prove_dev(ef, b["fst"], n, b["ts0"], b["pos"], b["secrets"], b["table"], b["entropy"], b["m"], b["nc"])
        finally:
            ef.close()
        oracle = {}
        for j in TH._sample_positions(n, np.random.default_rng(n)):
            oracle[j] = C.prove(b["cst"], b"thresholds", b["secrets"][j], np.concatenate([b["inst"][:, j], b["common"]]), b["entropy"][j].tobytes())[:3]
        return fresh, oracle

    fresh, oracle = _once(("prove", which, n), make)
    eh.set_option(OPT_DEV_OVERLAP, 2 if schedule == "latency" else 0)
    try:
        _fill(eh, CAP, word)
        got = _prove_dev(eh, b["fst"], n, b["ts0"], b["pos"], b["secrets"], b["table"], b["entropy"], b["m"], b["nc"])
        sched = eh.last_schedule()
    finally:
        eh.set_option(OPT_DEV_OVERLAP, 0)
    for k, v in expect.items():
        assert sched.get(k) == v, sched
    for j, (ec, er, ek) in oracle.items():
        assert got[0][j].tobytes() == ec.tobytes() and (got[1][j] == er).all() and (got[2][j] == ek).all(), "proof %d differs from the oracle's" % j
    for what, a, f in zip(("challenges", "responses", "commitments", "transcripts"), got, fresh):
        assert (a == f).all(), "%s differ from a fresh context's" % what


def _verify_mutants(n):
    """proof 0, proof N - 1 and the last index of every full 64-lane group"""
    return sorted({0, n - 1} | {g * 64 + 63 for g in range(n // 64)})


def _verify(eng, entry, b, n, responses, w):
    torch = _torch()
    d_ts, d_res = _dev(b["ts0"]), torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    if entry == "verify_compact":
        d_tbl, d_chal, d_resp = _dev(b["table"]), _dev(b["chal"]), _dev(responses)
        torch.cuda.synchronize()
        eng.fused_verify_compact_dev(b["fst"], n, b["pos"], d_ts.data_ptr(), d_tbl.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_res.data_ptr())
    else:
        d_tbl, d_resp, d_w = _dev(np.concatenate([b["table"], b["coms"].reshape(-1, 32)])), _dev(responses), _dev(w)
        torch.cuda.synchronize()
        eng.fused_verify_batchable_dev(b["fst"], n, b["pos"], d_ts.data_ptr(), d_tbl.data_ptr(), d_resp.data_ptr(), d_w.data_ptr(), d_res.data_ptr())
    eng.synchronize()
    return d_res.cpu().numpy(), d_ts.cpu().numpy()


VERIFY_FLOWS = [("verify_compact", "cmz"), ("verify_batchable", "dleq"), ("verify_batchable", "w64")]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("schedule", ("latency", "throughput"))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("flow", VERIFY_FLOWS, ids=lambda f: "%s-%s" % f)
def test_verify(engines, flow, n, schedule, word):
    eh, es = engines
    entry, which = flow
    b = _batch(es, which, n)
    mut = _verify_mutants(n)

    def make():
        bad = b["resp"].copy()
        bad[mut, 0, 0] ^= 1
        w = np.random.default_rng(n + 5).integers(0, 256, size=(n, b["nc"], 16), dtype=np.uint8)
        ef = _fresh(schedule)
        try:
            fresh = _verify(ef, entry, b, n, bad, w)
        finally:
            ef.close()
        return bad, w, fresh

    bad, w, fresh = _once(("verify", flow, n, schedule), make)
    eh.set_option(OPT_DEV_OVERLAP, 2 if schedule == "latency" else 0)
    try:
        _fill(eh, CAP, word)
        ok, _ = _verify(eh, entry, b, n, b["resp"], w)
        sched = eh.last_schedule()
        _fill(eh, CAP, word)
        got, ts = _verify(eh, entry, b, n, bad, w)
    finally:
        eh.set_option(OPT_DEV_OVERLAP, 0)
    assert sched.get("tr_lanes") == 2 and sched.get("tr_steps") == 1, sched   # a lane pair per proof; assemble + chain (the step form does not depend on the statement)
    if entry == "verify_compact":
        terms = n * (31 + 11)                                 # CMZ: 31 right-hand terms and 11 left-hand sides per proof
        assert sched.get("terms_split") == (1 if terms >= 1024 else 0), sched
        if terms >= 1024:
            # the statement classifier with paired terms (P rides on the C_i, V on Q).  The job's tables have 16 teeth (11 + N table points carry 30 N
            # terms), so P gets its table of multiples wherever verify_riders() allows one: on the throughput schedule, not on the latency one below 16,384 proofs
            assert sched.get("riders") == (1 if schedule == "throughput" else 0), sched
        else:
            assert "riders" not in sched, sched               # below 1,024 terms nothing is classified or paired
    else:
        assert (sched.get("straus_wins"), sched.get("straus_lanes")) == ((32, 1) if which == "dleq" else (0, 8)), sched
    assert not ok.any(), "honest proofs rejected: %s" % np.flatnonzero(ok)[:8]
    assert np.flatnonzero(got).tolist() == mut
    assert (got == fresh[0]).all() and (ts == fresh[1]).all(), "a fresh context gives other verdicts or transcripts"


# ---- batch verification ---------------------------------------------------------------------------------------------------------------
def _batch_verify(eng, b, K, n_each, responses, coms, w):
    """-> (out [K][32], status [K][2], transcripts); the caller's status words and output start as nonzero garbage"""
    torch = _torch()
    n = K * n_each
    fst = b["fst"]
    rows = fst.n_instance + len(fst._lhs)
    d_pts = torch.zeros((fst.n_static + rows * n, 32), dtype=torch.uint8, device="cuda:0")
    d_pts[: len(b["table"])] = _dev(b["table"])
    d_ts, d_coms, d_resp, d_w = _dev(b["ts0"]), _dev(coms), _dev(responses), _dev(w)
    d_out = torch.full((K, 32), 5, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((K, 2), 5, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if K == 1:
        eng.fused_batch_verify_dev(fst, n, b["pos"], d_ts.data_ptr(), d_pts.data_ptr(), d_coms.data_ptr(), d_resp.data_ptr(), d_w.data_ptr(), d_out.data_ptr(), d_st.data_ptr())
    else:
        eng.fused_batch_verify_many_dev(fst, K, n_each, b["pos"], d_ts.data_ptr(), d_pts.data_ptr(), d_coms.data_ptr(), d_resp.data_ptr(), d_w.data_ptr(),
                                        d_out.data_ptr(), d_st.data_ptr())
    eng.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy(), d_ts.cpu().numpy()


def _verdicts(out, st):
    """per batch: 0 = verified (the MSM is the identity and neither status word is set)"""
    return [int(out[k].any() or st[k].any()) for k in range(len(out))]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("n,shared,schedule", ((38, 0, "throughput"), (39, 1, "throughput"), (39, 1, "latency")))
def test_batch_verify_one_batch(engines, n, shared, schedule, word):
    """K = 1 on both status protocols: N = 38 (191 terms: two memsets), N = 39 (196 terms: the spare word behind the rejection flags) -- the
    latter also on the latency schedule, where the assemble pass clears that word BEFORE the fork and the decoder's atomicOr on the side
    stream meets it next to the transcript chain (`split` in batch_core)"""
    eh, es = engines
    b = _batch(es, "dleq", n)

    def make():
        rng = np.random.default_rng(n + 3)
        w = rng.integers(0, 256, size=(2, n, 16), dtype=np.uint8)
        bad = b["resp"].copy()
        bad[n // 2, 0, 0] ^= 1
        junk = b["coms"].copy()
        junk[n - 1, 1] = JUNK
        runs = {"good": (b["resp"], b["coms"]), "bad response": (bad, b["coms"]), "undecodable commitment": (b["resp"], junk)}
        oracle = {k: C.batch_verify(b["cst"], b"thresholds", n, b["inst"], b["common"], c, r, w) for k, (r, c) in runs.items()}
        assert oracle["good"] == 0 and oracle["bad response"] != 0 and oracle["undecodable commitment"] != 0
        ef = _fresh(schedule)
        try:
            fresh = {k: _batch_verify(ef, b, 1, n, r, c, w) for k, (r, c) in runs.items()}
        finally:
            ef.close()
        return w, runs, fresh

    w, runs, fresh = _once(("batch1", n, schedule), make)
    for name, (r, c) in runs.items():
        eh.set_option(OPT_DEV_OVERLAP, 2 if schedule == "latency" else 0)
        try:
            _fill(eh, CAP, word)
            out, st, ts = _batch_verify(eh, b, 1, n, r, c, w)
            sched = eh.last_schedule()
        finally:
            eh.set_option(OPT_DEV_OVERLAP, 0)
        assert sched.get("status_shared") == shared and sched.get("opt_pip") == shared, sched
        assert sched.get("tr_steps") == 1 and sched.get("tr_lanes") == 2, sched       # (the fork needs the step form: its assemble pass owns the flag word)
        if name == "good":
            assert not out.any() and not st.any(), (name, out, st)
        elif name == "bad response":
            assert out.any() and not st.any(), (name, out, st)            # the MSM is not the identity; nothing else is wrong
        else:
            assert st.tolist() == [[1, 0]] and not out.any(), (name, out, st)   # a decode failure: flagged, output cleared
        for what, a, f in zip(("output", "status", "transcripts"), (out, st, ts), fresh[name]):
            assert (a == f).all(), "%s: %s differs from a fresh context's" % (name, what)


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
def test_batch_verify_three_batches(engines, word):
    """K = 3 batches of 39 proofs, a wrong response in batch 1 only: verdicts (0, 1, 0)"""
    eh, es = engines
    K, n_each = 3, 39
    n = K * n_each
    b = _batch(es, "dleq", n)

    def make():
        w = np.random.default_rng(n + 3).integers(0, 256, size=(2, n, 16), dtype=np.uint8)
        bad = b["resp"].copy()
        bad[n_each + n_each - 1, 0, 0] ^= 1                                    # the last proof of batch 1
        want = [int(C.batch_verify(b["cst"], b"thresholds", n_each, np.ascontiguousarray(b["inst"][:, k * n_each:(k + 1) * n_each]), b["common"],
                                   b["coms"][k * n_each:(k + 1) * n_each], bad[k * n_each:(k + 1) * n_each],
                                   np.ascontiguousarray(w[:, k * n_each:(k + 1) * n_each])) != 0) for k in range(K)]
        assert want == [0, 1, 0]
        ef = _fresh()
        try:
            fresh = _batch_verify(ef, b, K, n_each, bad, b["coms"], w)
        finally:
            ef.close()
        return w, bad, fresh

    w, bad, fresh = _once(("batch3",), make)
    _fill(eh, CAP, word)
    out, st, ts = _batch_verify(eh, b, K, n_each, b["resp"], b["coms"], w)
    assert eh.last_schedule().get("status_shared") == 1
    assert _verdicts(out, st) == [0, 0, 0], (out[:, :4], st)
    _fill(eh, CAP, word)
    out, st, ts = _batch_verify(eh, b, K, n_each, bad, b["coms"], w)
    assert _verdicts(out, st) == [0, 1, 0] and not st.any(), (out[:, :4], st)
    for what, a, f in zip(("output", "status", "transcripts"), (out, st, ts), fresh):
        assert (a == f).all(), "%s differs from a fresh context's" % what


# ---- zkp_batch_check: the coefficient build on the device with a carve of its own (partial sums, incidence words, n + 1 rows of operands) ----
def _batch_check(eng, b, n, minus_c, responses, coms, w):
    """-> (out [32], status, coefficient vector [n_static + (n_instance + n_constraints) n][32]); out and status start as nonzero garbage"""
    import ctypes
    fst = b["fst"]
    total = fst.n_static + (fst.n_instance + len(fst._lhs)) * n
    out, status, coeffs = np.full(32, 5, np.uint8), ctypes.c_int(5), np.full((total, 32), 5, np.uint8)
    keep = [np.ascontiguousarray(a, np.uint8) for a in (minus_c, responses, w, b["common"], b["inst"], coms)]
    rc = eng._lib.zkp_batch_check(eng._h, ctypes.byref(fst.c.shape), n, *(a.ctypes.data for a in keep), out.ctypes.data, ctypes.byref(status), coeffs.ctypes.data)
    assert rc == 0, eng._lib.zkp_last_error()
    return out, status.value, coeffs


def _batch_coefficients(fst, n, minus_c, responses, w):
    """batch_verifier.rs:173-223 in Python integers: static coefficients, then the matrix row-major (instance rows, then one row -r_ij per constraint)"""
    ns, ni, nc = fst.n_static, fst.n_instance, len(fst._lhs)
    val = lambda row: int.from_bytes(bytes(row), "little")
    static, mat = [0] * ns, [[0] * n for _ in range(ni + nc)]

    def add(pid, j, v):
        if pid < ns:
            static[pid] = (static[pid] + v) % M.L
        else:
            mat[pid - ns][j] = (mat[pid - ns][j] + v) % M.L
    for j in range(n):
        mc = val(minus_c[j])
        for i in range(nc):
            r = val(w[i][j])
            add(int(fst._lhs[i]), j, r * mc)
            for t in range(int(fst._off[i]), int(fst._off[i + 1])):
                add(int(fst._pt[t]), j, r * val(responses[j][int(fst._sc[t])]))
            mat[ni + i][j] = (M.L - r) % M.L
    return static + [v for row in mat for v in row]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("n,pip", ((38, 0), (39, 1), (257, 1)))
def test_batch_check(engines, n, pip, word):
    """N = 38 (191 operands: the term path), 39 (196: Pippenger) and 257 (two blocks of partial sums for the static coefficient): the coefficient
    vector equals Python integers, the point is the C oracle's MSM over it, the verdicts are the C oracle's batch verifier's"""
    eh, es = engines
    b = _batch(es, "dleq", n)
    fst = b["fst"]

    def make():
        from tests.test_host_scalar_ops import rows
        rng = np.random.default_rng(n + 4)
        w = rng.integers(0, 256, size=(2, n, 16), dtype=np.uint8)
        minus_c = rows([(M.L - int.from_bytes(bytes(c), "little")) % M.L for c in b["chal"]])
        bad = b["resp"].copy()
        bad[n // 2, 0, 0] ^= 1
        junk = b["coms"].copy()
        junk[n - 1, 1] = JUNK
        runs = {"good": (b["resp"], b["coms"]), "bad response": (bad, b["coms"]), "undecodable commitment": (b["resp"], junk)}
        want = {}
        for k, (r, c) in runs.items():
            verdict = C.batch_verify(b["cst"], b"thresholds", n, b["inst"], b["common"], c, r, w)
            coeffs = rows(_batch_coefficients(fst, n, minus_c, r, w))
            pts = np.concatenate([b["common"], b["inst"].reshape(-1, 32), np.ascontiguousarray(c.transpose(1, 0, 2)).reshape(-1, 32)])
            want[k] = (verdict, coeffs, C.msm_optional(coeffs, pts))
        assert want["good"][0] == 0 and want["good"][2] == IDENTITY and want["bad response"][0] != 0 and want["bad response"][2] not in (None, IDENTITY)
        assert want["undecodable commitment"][0] != 0 and want["undecodable commitment"][2] is None
        ef = _fresh()
        try:
            fresh = {k: _batch_check(ef, b, n, minus_c, r, c, w) for k, (r, c) in runs.items()}
        finally:
            ef.close()
        return w, minus_c, runs, want, fresh

    w, minus_c, runs, want, fresh = _once(("batch_check", n), make)
    for name, (r, c) in runs.items():
        _fill(eh, CAP, word)
        out, st, coeffs = _batch_check(eh, b, n, minus_c, r, c, w)
        assert eh.last_schedule().get("opt_pip") == pip, eh.last_schedule()
        _, want_coeffs, want_pt = want[name]
        assert (coeffs == want_coeffs).all(), "%s: coefficients differ in rows %s" % (name, np.flatnonzero((coeffs != want_coeffs).any(axis=1))[:8])
        if want_pt is None:
            assert st == 1 and not out.any(), (name, st, out)
        else:
            assert st == 0 and out.tobytes() == want_pt, (name, st, out)
        for what, a, f in zip(("output", "status", "coefficients"), (out, st, coeffs), fresh[name]):
            assert np.array_equal(a, f), "%s: %s differs from a fresh context's" % (name, what)


# ---- one ragged call per flow: 65 proofs, three STROBE position classes ---------------------------------------------------------------
def _ragged_inputs(es):
    def make():
        from zkp_amd import toolbox as T
        n = 65
        b = _batch(es, "dleq", n)
        rng = np.random.default_rng(65)
        lens = [(10, 50, 120)[j % 3] for j in range(n)]
        ts0 = T.append_messages(b"residue", b"msg", [rng.bytes(k) for k in lens])
        assert len({bytes(r[200:203]) for r in ts0}) == 3
        st = T.dleq_module().statement
        host = T.HostEngine()
        entropy = b["entropy"]
        ts = ts0.copy()
        chal, resp, coms = T.prove_batch(host, st, ts, b["secrets"], b["inst"], b["common"], entropy)
        mut = _verify_mutants(n)
        bad = resp.copy()
        bad[mut, 0, 0] ^= 1
        w_each = rng.integers(0, 256, size=(n, 2, 16), dtype=np.uint8)
        w = rng.integers(0, 256, size=(2, n, 16), dtype=np.uint8)
        one = resp.copy()
        one[2 * 13 + 12, 0, 0] ^= 1                                            # the last proof of batch 2 of 5
        tv = ts0.copy()
        want = dict(prove=(chal, resp, coms, ts),
                    compact=(T.verify_compact_batch(host, st, tv, b["inst"], b["common"], chal, bad), tv),
                    each=T.verify_batchable_each(host, st, ts0.copy(), b["inst"], b["common"], coms, bad, w_each),
                    many=T.batch_verify_many(host, st, 5, ts0.copy(), b["inst"], b["common"], coms, one, w))
        assert np.flatnonzero(want["compact"][0]).tolist() == mut and np.flatnonzero(want["each"]).tolist() == mut and want["many"].tolist() == [0, 0, 1, 0, 0]
        th = ts0.copy()
        want["hash"] = (T.hash_to_group(None, th), th)
        return dict(b=b, ts0=ts0, entropy=entropy, bad=bad, one=one, w_each=w_each, w=w, want=want)
    return _once(("ragged",), make)


def _ragged_call(eng, flow, r):
    b, want = r["b"], r["want"]
    fst, ts = b["fst"], r["ts0"].copy()
    chal, resp, coms, _ = want["prove"]
    if flow == "prove":
        got = eng.fused_prove_ragged(fst, ts, b["secrets"], b["inst"], b["common"], r["entropy"])
        assert got[3] == 0
        return got[:3] + (ts,)
    if flow == "compact":
        return eng.fused_verify_compact_ragged(fst, ts, b["inst"], b["common"], chal, r["bad"]), ts
    if flow == "each":
        return (eng.fused_verify_batchable_ragged(fst, ts, b["inst"], b["common"], coms, r["bad"], r["w_each"]),)
    if flow == "many":
        return (eng.fused_batch_verify_many_ragged(fst, 5, ts, b["inst"], b["common"], coms, r["one"], r["w"]),)
    return eng.fused_hash_to_group_ragged(ts), ts


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("flow", ("prove", "compact", "each", "many", "hash"))
def test_ragged(engines, flow, word):
    eh, es = engines
    r = _ragged_inputs(es)

    def make():
        ef = _fresh()
        try:
            return _ragged_call(ef, flow, r)
        finally:
            ef.close()

    fresh = _once(("ragged", flow), make)
    _fill(eh, CAP, word)
    got = _ragged_call(eh, flow, r)
    sched = eh.last_schedule()
    assert sched.get("ragged_classes") == 3, sched
    want = r["want"][flow]
    want = want if isinstance(want, tuple) else (want,)
    for a, e, f in zip(got, want, fresh):
        a, e, f = np.asarray(a), np.asarray(e), np.asarray(f)
        if a.ndim == 2 and a.shape[1] == 208:                                  # transcripts: the state and the position (bytes 203 .. 207 are padding)
            a, e, f = a[:, :203], e[:, :203], f[:, :203]
        assert (a == e).all(), "%s differs from the host backend" % flow
        assert (a == f).all(), "%s differs from a fresh context" % flow


# ---- the calls that draw into the workspace or stage through it -----------------------------------------------------------------------
KEY, NONCE = bytes(range(32)), 0x1122334455667788


def _other_inputs():
    def make():
        rng = np.random.default_rng(257)
        n = 257
        uni = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        msgs = [rng.bytes(int(k)) for k in rng.integers(0, 300, size=n)]
        want = {"from_uniform_bytes": np.frombuffer(b"".join(C.from_uniform_bytes(u.tobytes()) for u in uni), np.uint8).reshape(n, 32),
                "hash_from_bytes_sha512": np.frombuffer(b"".join(C.from_uniform_bytes(hashlib.sha512(m_).digest()) for m_ in msgs), np.uint8).reshape(n, 32),
                "scalar_random": [int.from_bytes(chacha_block(KEY, i, NONCE), "little") % M.L for i in range(n)],
                "scalar_hash_from_bytes_sha512": want_hash(msgs)}
        return n, uni, msgs, want
    return _once(("other",), make)


def _other_call(eng, op, n, uni, msgs):
    if op == "from_uniform_bytes":
        return eng.from_uniform_bytes(uni)
    if op == "hash_from_bytes_sha512":
        return eng.hash_from_bytes_sha512(msgs)
    if op == "scalar_random":
        return eng.scalar_random(n, KEY, NONCE)
    return eng.scalar_hash_from_bytes_sha512(msgs)


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("op", ("from_uniform_bytes", "hash_from_bytes_sha512", "scalar_random", "scalar_hash_from_bytes_sha512"))
def test_other_calls(engines, op, word):
    eh, _ = engines
    n, uni, msgs, want = _other_inputs()

    def make():
        ef = _fresh()
        try:
            return _other_call(ef, op, n, uni, msgs)
        finally:
            ef.close()

    fresh = _once(("other", op), make)
    _fill(eh, CAP, word)
    got = _other_call(eh, op, n, uni, msgs)
    if op.startswith("scalar"):
        assert ints(got) == want[op]
    else:
        assert (got == want[op]).all()
    assert (got == fresh).all(), "a fresh context computes other bytes"


# ---- the transcript calls, the rest of the scalar calls and the aligned hash to group: staged through the workspace by their host-pointer forms ----
def _strobe_inputs(n):
    """n transcripts at a mix of positions (row 0 at 165, the last byte of a block) and what the calls below take besides them"""
    def make():
        rng = np.random.default_rng(1000 + n)
        msgs = [rng.bytes((0, 60, 167)[j % 3]) for j in range(n)]
        wit, ent = rng.integers(0, 256, size=(n, 2, 32), dtype=np.uint8), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        pts = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        pts[:, 0] |= 1
        pts[[1, n // 2]] = 0                                                     # the identity's encoding: refused under validate
        ts = PH.states(n, n)
        assert ts[0, 200] == 165 and len(set(ts[:, 200].tolist())) >= 40
        return dict(ts=ts, msgs=msgs, wit=wit, ent=ent, pts=pts)
    return _once(("strobe", n), make)


STROBE_OPS = ("append_message", "challenge_bytes_0", "challenge_bytes_32", "challenge_bytes_200", "witness_rng_scalars", "witness_rng_bytes",
              "challenge_scalars", "append_points", "append_points_validate")


def _strobe_want(op, d):
    """oracle.model's Merlin in Python, from the blob: -> the tuple _strobe_call returns"""
    ts = d["ts"]
    if op == "append_message":
        return (PH.model_append(ts, b"msg", d["msgs"]),)
    if op.startswith("challenge_bytes"):
        return PH.model_challenge(ts, b"chal", int(op.rsplit("_", 1)[1]))
    if op.startswith("witness_rng"):
        mode, count = (0, 2) if op.endswith("scalars") else (1, 200)
        return PH.model_rng(ts, b"w", d["wit"], d["ent"], mode, count), ts
    if op == "challenge_scalars":
        return PH.model_challenge_scalars(ts, b"chal")
    return PH.model_append_points(ts, b"blindcom", b"A", d["pts"], op.endswith("validate"))


def _strobe_call(eng, op, d):
    from zkp_amd.engine import messages_csr
    ts = d["ts"].copy()
    if op == "append_message":
        return (eng.transcripts_append_message(ts, b"msg", *messages_csr(d["msgs"])),)
    if op.startswith("challenge_bytes"):
        return eng.transcripts_challenge_bytes(ts, b"chal", int(op.rsplit("_", 1)[1])), ts
    if op.startswith("witness_rng"):
        mode, count = (0, 2) if op.endswith("scalars") else (1, 200)
        return eng.transcripts_witness_rng(ts, b"w", d["wit"], d["ent"], mode, count), ts
    if op == "challenge_scalars":
        return eng.transcripts_challenge_scalars(ts, b"chal"), ts
    return eng.transcripts_append_points(ts, b"blindcom", b"A", d["pts"], op.endswith("validate")), ts


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("n", (65, 257))
@pytest.mark.parametrize("op", STROBE_OPS)
def test_transcript_calls(engines, op, n, word):
    eh, _ = engines
    d = _strobe_inputs(n)

    def make():
        ef = _fresh()
        try:
            return _strobe_want(op, d), _strobe_call(ef, op, d)
        finally:
            ef.close()

    want, fresh = _once(("strobe", op, n), make)
    if op == "append_points_validate":
        assert np.flatnonzero(want[0]).tolist() == [1, n // 2]
    _fill(eh, CAP, word)
    got = _strobe_call(eh, op, d)
    for what, a, e, f in zip(("result", "transcripts"), got, want, fresh):
        assert a.shape == e.shape and (a == e).all(), "%s differs from oracle.model: rows %s" % (what, np.flatnonzero((a != e).reshape(n, -1).any(axis=1))[:8])
        assert (a == f).all(), "%s: a fresh context computes other bytes" % what


SCALAR_OPS = ["invert", "from_wide"] + ["muladd_%d%d%d" % s for s in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))]


def _scalar_inputs(n):
    def make():
        from tests.scalar_edge_cases import VALUES, random_256
        from tests.test_host_scalar_ops import WIDE_EDGES, muladd_operands, rows
        inv = ([0, 1, M.L - 1, M.L, M.L + 1, 2**256 - 1] + VALUES + random_256(n, n))[:n]
        rng = np.random.default_rng(n)
        wide = (WIDE_EDGES + [int.from_bytes(rng.bytes(64), "little") for _ in range(n)])[:n]
        recs = muladd_operands()[:n]
        return dict(inv=inv, wide=wide, recs=recs, a=rows([r[0] for r in recs]), b=rows([r[1] for r in recs]), c=rows([r[2] for r in recs]),
                    inv_rows=rows(inv), wide_rows=rows(wide, 64))
    return _once(("scalars", n), make)


def _scalar_call(eng, op, d):
    if op == "invert":
        return eng.scalar_invert(d["inv_rows"])
    if op == "from_wide":
        return eng.scalar_from_wide(d["wide_rows"])
    sa, sb, sc = (int(ch) for ch in op[-3:])
    n = len(d["a"])
    out = np.zeros((n, 32), np.uint8)
    p = lambda x: x.ctypes.data
    assert eng._lib.zkp_sc_muladd(eng._h, n, p(d["a"]), sa, p(d["b"]), sb, p(d["c"]), sc, p(out)) == 0
    return out


def _scalar_want(op, d):
    if op == "invert":
        return [pow(v % M.L, M.L - 2, M.L) for v in d["inv"]]
    if op == "from_wide":
        return [v % M.L for v in d["wide"]]
    sa, sb, sc = (int(ch) for ch in op[-3:])
    r = d["recs"]
    return [(r[i * sa][0] * r[i * sb][1] + r[i * sc][2]) % M.L for i in range(len(r))]


SCALAR_PARAMS = [(op, n) for op in SCALAR_OPS for n in (65, 257) if n == 257 or op in ("invert", "from_wide", "muladd_111")]


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("op,n", SCALAR_PARAMS, ids=["%s-%d" % p for p in SCALAR_PARAMS])
def test_scalar_calls(engines, op, n, word):
    eh, _ = engines
    d = _scalar_inputs(n)

    def make():
        ef = _fresh()
        try:
            return _scalar_call(ef, op, d)
        finally:
            ef.close()

    fresh = _once(("scalars", op, n), make)
    _fill(eh, CAP, word)
    got = _scalar_call(eh, op, d)
    assert ints(got) == _scalar_want(op, d)
    assert (got == fresh).all(), "a fresh context computes other bytes"


def _aligned_hash(eng, ts0):
    ts, out = ts0.copy(), np.zeros((len(ts0), 32), np.uint8)
    assert eng._lib.zkp_fused_hash_to_group(eng._h, len(ts), ts.ctypes.data, b"output", out.ctypes.data) == 0
    return out, ts


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
@pytest.mark.parametrize("n", (65, 257))
def test_aligned_hash_to_group(engines, n, word):
    """zkp_fused_hash_to_group on transcripts that stand at ONE position (test_ragged has the ragged form), above the toolbox's fused threshold"""
    eh, _ = engines

    def make():
        from zkp_amd import toolbox as T
        assert n >= T.get_fused_min_batch()
        rng = np.random.default_rng(n + 11)
        ts0 = T.append_messages(b"residue", b"msg", [rng.bytes(20) for _ in range(n)])
        assert len({bytes(r[200:203]) for r in ts0}) == 1 and len({bytes(r) for r in ts0}) == n
        wide, adv = PH.model_challenge(ts0, b"output", 64)
        want = np.frombuffer(b"".join(C.from_uniform_bytes(w.tobytes()) for w in wide), np.uint8).reshape(n, 32)
        ef = _fresh()
        try:
            fresh = _aligned_hash(ef, ts0)
        finally:
            ef.close()
        return ts0, (want, adv), fresh

    ts0, want, fresh = _once(("aligned_hash", n), make)
    _fill(eh, CAP, word)
    got = _aligned_hash(eh, ts0)
    for what, a, e, f in zip(("points", "transcripts"), got, want, fresh):
        assert (a[:, :203] == e[:, :203]).all(), "%s differ from oracle.model and the C oracle's map" % what
        assert (a == f).all(), "%s: a fresh context computes other bytes" % what


@pytest.mark.parametrize("word", WORDS, ids=lambda w: "fill%x" % w)
def test_decode_check_and_encode_many(engines, word):
    """valid encodings with the ones RFC 9496 rejects between them: statuses = the C oracle's, and encode(decode(P)) = P"""
    eh, _ = engines

    def make():
        from tests import point_mul_cases as PC
        pts = PC.tiled(PC.pair_operands()[1][-120:], 257)
        want = C.decode_check(pts)
        assert 0 < int(want.sum()) < len(pts)
        ef = _fresh()
        try:
            st, xyzt = ef.decode_check(pts, want_coords=True)
            fresh = (st, ef.encode_many(xyzt))
        finally:
            ef.close()
        return pts, want, fresh

    pts, want, fresh = _once(("decode_encode",), make)
    _fill(eh, CAP, word)
    st, xyzt = eh.decode_check(pts, want_coords=True)
    assert (st == want).all() and (st == fresh[0]).all()
    _fill(eh, CAP, word)
    enc = eh.encode_many(xyzt)
    ok = want == 0
    assert (enc[ok] == pts[ok]).all() and (enc[ok] == fresh[1][ok]).all()     # (the coordinates of a row that does not decode are unspecified)


def test_fill_is_refused_during_a_capture_and_moves_the_workspace_generation(engines):
    """the hook grows the workspace through the path every call takes: a graph captured before a growing fill is stale afterwards"""
    from zkp_amd.engine import Engine, ZkpError
    torch = _torch()
    e = Engine(0, test_hooks=True)
    try:
        d_out = torch.zeros((4, 32), dtype=torch.uint8, device="cuda:0")
        msgs = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        offs = torch.arange(5, dtype=torch.int64, device="cuda:0") * 4
        torch.cuda.synchronize()
        e.debug_fill_workspace(1 << 16, 3)
        e.hash_from_bytes_sha512_dev(4, msgs.data_ptr(), 16, offs.data_ptr(), d_out.data_ptr())     # (its digests go through the workspace)
        e.synchronize()
        want = d_out.cpu().numpy().copy()
        with e.capture() as cap:
            with pytest.raises(ZkpError):
                e.debug_fill_workspace(0, 0)
            e.hash_from_bytes_sha512_dev(4, msgs.data_ptr(), 16, offs.data_ptr(), d_out.data_ptr())
        d_out.zero_()
        e.debug_fill_workspace(0, 0xFFFFFFFF)                   # no growth: the graph stays valid
        cap.graph.launch()
        e.synchronize()
        assert (d_out.cpu().numpy() == want).all()
        e.debug_fill_workspace(1 << 20, 0)                      # growth: stale from here on
        with pytest.raises(ZkpError):
            cap.graph.launch()
        cap.graph.close()
    finally:
        e.close()

"""(helper module of tests/test_gpu_statement_shapes.py and tests/test_host_backend.py)
Statement shapes the constraint API allows and the reference's own tests never build (missing 4): a STATIC point as a
constraint's left-hand side (batch_verifier.rs:156-160, 186-188: its r * (-c) is summed over the batch into static_coeffs), one point as
left-hand side of two constraints, a point that is left-hand side of one constraint and right-hand side of another, a repeated term, and
statements of 64 constraints (the second reading of BASELINE configs[4]).  Each through prove / verify_compact / verify_batchable (per
proof) / batch_verify / batch_verify_many, on the fused device route and the host-transcript route, against the oracle's restatement of
prover.rs / verifier.rs / batch_verifier.rs -- proofs byte for byte, the batch verifier's operand scalars (static_coeffs first) scalar for
scalar."""
import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from zkp_amd import toolbox as T
from tests.test_gpu_toolbox import BASEPOINT

NEVER = 0xFFFFFFFF
L = M.L


def _sc(v: int) -> np.ndarray:
    return np.frombuffer((v % L).to_bytes(32, "little"), np.uint8)


def _rand_scalars(rng, k):
    s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    s[:, 31] &= 0x0f
    return s


def _ints(a):
    return [int.from_bytes(x.tobytes(), "little") for x in a.reshape(-1, 32)]


def _mul_base(scalars_int):
    """[k] ints -> [k][32] encodings of s * B"""
    base = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32)
    k = len(scalars_int)
    sc = np.stack([_sc(v) for v in scalars_int])
    pts, st = C.msm_many(np.arange(k + 1, dtype=np.uint32), sc, np.zeros(k, np.uint32), base, 0)
    assert not st.any()
    return pts


class Shape:
    """points: [(name, is_common)] in allocation order; cons: [(lhs name, [(secret name, point name)])];
    every point is d * B for a known discrete log d (common: one int, instance: [n] ints), so any left-hand side can be computed"""

    def __init__(self, label, secret_names, points, cons):
        self.label, self.secret_names, self.points, self.cons = label, secret_names, points, cons

    def build(self):
        st = T.Statement(self.label)
        sv = {s: st.add_secret(s.encode()) for s in self.secret_names}
        pv = {p: st.add_point(p.encode(), c) for p, c in self.points}
        for lhs, lc in self.cons:
            st.constrain(pv[lhs], [(sv[s], pv[p]) for s, p in lc])
        cst = C.Statement(self.label, self.secret_names, self.points, self.cons)
        return st, cst


def _materialise(shape, n, secrets_int, dlog):
    """secrets_int: name -> [n] ints; dlog: point name -> int (common) or [n] ints (instance), left-hand sides included"""
    m = len(shape.secret_names)
    secrets = np.zeros((n, m, 32), np.uint8)
    for i, s in enumerate(shape.secret_names):
        secrets[:, i] = np.stack([_sc(v) for v in secrets_int[s]])
    inst_names = [p for p, c in shape.points if not c]
    common_names = [p for p, c in shape.points if c]
    common = _mul_base([dlog[p] for p in common_names]) if common_names else np.zeros((0, 32), np.uint8)
    inst = np.stack([_mul_base(list(dlog[p])) for p in inst_names]) if inst_names else np.zeros((0, n, 32), np.uint8)
    # the statement is true: every constraint holds in the exponent
    for lhs, lc in shape.cons:
        for j in (0, n - 1):
            want = sum(secrets_int[s][j] * (dlog[p] if isinstance(dlog[p], int) else dlog[p][j]) for s, p in lc) % L
            have = dlog[lhs] if isinstance(dlog[lhs], int) else dlog[lhs][j]
            assert want == have % L, (lhs, j)
    return secrets, np.ascontiguousarray(inst), np.ascontiguousarray(common)


def _fresh(label, n):
    return np.stack([T.Transcript(label).state] * n)


def _check_all_flows(eng, shape, n, secrets, inst, common, seed, oracle_samples=(0, -1)):
    st, cst = shape.build()
    rng = np.random.default_rng(seed)
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    nc = st.nc
    w = rng.integers(0, 256, size=(nc, n, 16), dtype=np.uint8)
    tl = b"shapes"
    out = {}
    for route, thr in (("host", NEVER), ("fused", 0)):
        T.set_fused_min_batch(thr)
        try:
            ts = _fresh(tl, n)
            chal, resp, coms = T.prove_batch(eng, st, ts, secrets, inst, common, entropy)
            ts2 = _fresh(tl, n)
            res = T.verify_compact_batch(eng, st, ts2, inst, common, chal, resp)
            ts3 = _fresh(tl, n)
            ok, coeffs = T.batch_verify_coeffs(eng, st, ts3, inst, common, coms, resp, w)
            ts4 = _fresh(tl, n)
            each = T.verify_batchable_each(eng, st, ts4, inst, common, coms, resp, np.ascontiguousarray(w.transpose(1, 0, 2)))
            bad = resp.copy()
            bad[n // 2, 0, 0] ^= 1
            ts5 = _fresh(tl, n)
            res_bad = T.verify_compact_batch(eng, st, ts5, inst, common, chal, bad)
            ts6 = _fresh(tl, n)
            each_bad = T.verify_batchable_each(eng, st, ts6, inst, common, coms, bad, np.ascontiguousarray(w.transpose(1, 0, 2)))
            verd = verd_bad = None
            if n % 2 == 0 and n >= 2:
                ts7 = _fresh(tl, n)
                verd = T.batch_verify_many(eng, st, 2, ts7, inst, common, coms, resp, w)
                ts8 = _fresh(tl, n)
                verd_bad = T.batch_verify_many(eng, st, 2, ts8, inst, common, coms, bad, w)
            ts9 = _fresh(tl, n)
            T.batch_verify(eng, st, ts9, inst, common, coms, resp, w)                       # raises on failure
            ts10 = _fresh(tl, n)
            with pytest.raises(T.VerificationFailure):
                T.batch_verify(eng, st, ts10, inst, common, coms, bad, w)
        finally:
            T.set_fused_min_batch(32)
        assert ok and not res.any() and not each.any(), route
        assert res_bad[n // 2] == 1 and res_bad.sum() == 1 and each_bad[n // 2] == 1 and each_bad.sum() == 1, route
        if verd is not None:
            assert verd.tolist() == [0, 0] and verd_bad.tolist() == [0, 1], route
        out[route] = (chal, resp, coms, ts[:, :203], ts2[:, :203], coeffs, ts3[:, :203], ts4[:, :203])
    for a, b in zip(out["host"], out["fused"]):
        assert a.shape == b.shape and (a == b).all()
    chal, resp, coms = out["fused"][:3]
    # the oracle: proofs byte for byte (its point list is the allocation order) ...
    names = [p for p, _ in shape.points]
    inst_names = [p for p, c in shape.points if not c]
    common_names = [p for p, c in shape.points if c]
    for j in oracle_samples:
        j = j % n
        pts_j = np.stack([common[common_names.index(p)] if c else inst[inst_names.index(p)][j] for p, c in shape.points])
        ec, er, ek, _ = C.prove(cst, tl, secrets[j], pts_j, entropy[j].tobytes())
        assert chal[j].tobytes() == ec.tobytes() and (resp[j] == er).all() and (coms[j] == ek).all(), j
        assert C.verify_compact(cst, tl, pts_j, chal[j], resp[j]) == 0
    # ... and the batch verifier's operand list: static_coeffs (batch_verifier.rs:186-188, 198) first, then the row-major matrix
    if n <= 512:
        rc, osc, _ = C.batch_verify(cst, tl, n, inst, common, coms, resp, w, want_msm_inputs=True)
        assert rc == 0 and (osc == out["fused"][5]).all()
        assert C.batch_verify(cst, tl, n, inst, common, coms, resp, w) == 0
    return out["fused"]


def _shape_case(name, n, rng):
    """-> (Shape, secrets_int, dlog)"""
    r = lambda: int.from_bytes(rng.bytes(32), "little") % L
    rn = lambda: [r() for _ in range(n)]
    g, h = r(), r()
    if name == "static_lhs_unused_on_rhs":
        # K = k G with K, G static: the same statement in every proof of the batch (an issuer key); K is on no right-hand side
        k, x = r(), rn()
        shape = Shape(b"static lhs", ["k", "x"], [("G", True), ("H", True), ("K", True), ("A", False)], [("K", [("k", "G")]), ("A", [("x", "H")])])
        return shape, {"k": [k] * n, "x": x}, {"G": g, "H": h, "K": k * g % L, "A": [xi * h % L for xi in x]}
    if name == "static_lhs_used_on_rhs":
        # ... and the static left-hand side is the base of the per-proof constraint; statics allocated AFTER the instance point
        k, x = r(), rn()
        shape = Shape(b"static lhs 2", ["x", "k"], [("A", False), ("G", True), ("K", True)], [("A", [("x", "K")]), ("K", [("k", "G")])])
        return shape, {"k": [k] * n, "x": x}, {"G": g, "K": k * g % L, "A": [xi * k * g % L for xi in x]}
    if name == "static_lhs_twice":
        # one static point as left-hand side of two constraints: K = k G = k' H
        k = r()
        k2 = k * g * pow(h, -1, L) % L
        x = rn()
        shape = Shape(b"static lhs twice", ["k", "k2", "x"], [("G", True), ("H", True), ("K", True), ("A", False)],
                      [("K", [("k", "G")]), ("A", [("x", "G"), ("k", "H")]), ("K", [("k2", "H")])])
        return shape, {"k": [k] * n, "k2": [k2] * n, "x": x}, {"G": g, "H": h, "K": k * g % L, "A": [(xi * g + k * h) % L for xi in x]}
    if name == "instance_lhs_twice":
        # A = x G and A = y H for one instance point A
        x = rn()
        y = [xi * g * pow(h, -1, L) % L for xi in x]
        shape = Shape(b"lhs twice", ["x", "y"], [("A", False), ("G", True), ("H", True)], [("A", [("x", "G")]), ("A", [("y", "H")])])
        return shape, {"x": x, "y": y}, {"G": g, "H": h, "A": [xi * g % L for xi in x]}
    if name == "lhs_is_rhs_elsewhere":
        # A = x G ; B = y A + x G   (A: left-hand side of the first, right-hand side of the second)
        x, y = rn(), rn()
        a = [xi * g % L for xi in x]
        shape = Shape(b"lhs and rhs", ["x", "y"], [("G", True), ("A", False), ("B", False)], [("A", [("x", "G")]), ("B", [("y", "A"), ("x", "G")])])
        return shape, {"x": x, "y": y}, {"G": g, "A": a, "B": [(yi * ai + xi * g) % L for xi, yi, ai in zip(x, y, a)]}
    if name == "repeated_term":
        # the same (scalar, point) term twice in one constraint, and a constraint whose terms all name one point: A = x G + x G + y G
        x, y = rn(), rn()
        shape = Shape(b"repeated term", ["x", "y"], [("A", False), ("G", True)], [("A", [("x", "G"), ("x", "G"), ("y", "G")])])
        return shape, {"x": x, "y": y}, {"G": g, "A": [(2 * xi + yi) * g % L for xi, yi in zip(x, y)]}
    if name == "only_static_points":
        # no instance point at all: every proof of the batch proves the same two static relations (ni = 0: the matrix has commitment rows only)
        k, k2 = r(), r()
        shape = Shape(b"only statics", ["k", "k2"], [("G", True), ("H", True), ("K", True), ("K2", True)], [("K", [("k", "G")]), ("K2", [("k2", "H"), ("k", "K")])])
        return shape, {"k": [k] * n, "k2": [k2] * n}, {"G": g, "H": h, "K": k * g % L, "K2": (k2 * h + k * k * g) % L}
    raise KeyError(name)


SHAPES = ["static_lhs_unused_on_rhs", "static_lhs_used_on_rhs", "static_lhs_twice", "instance_lhs_twice", "lhs_is_rhs_elsewhere", "repeated_term", "only_static_points"]


def _w64_constraints_shape(terms_per_constraint):
    """the second reading of BASELINE configs[4] ("64-constraint Schnorr"): 64 constraints Q_i = x_i G_i (+ y_i H), generators static"""
    xs = ["x_%d" % i for i in range(64)]
    ys = ["y_%d" % i for i in range(64)] if terms_per_constraint == 2 else []
    points = [("Q_%d" % i, False) for i in range(64)] + [("G_%d" % i, True) for i in range(64)] + ([("H", True)] if ys else [])
    cons = [("Q_%d" % i, [("x_%d" % i, "G_%d" % i)] + ([("y_%d" % i, "H")] if ys else [])) for i in range(64)]
    return Shape(b"W64 constraints", xs + ys, points, cons)


def w64_constraints_case(n, tpc, rng):
    """-> (shape, secrets, inst, common) of n proofs of the 64-constraint statement with tpc terms per constraint"""
    shape = _w64_constraints_shape(tpc)
    r = lambda: int.from_bytes(rng.bytes(32), "little") % L
    g = [r() for _ in range(64)]
    h = r()
    secrets_int = {"x_%d" % i: [r() for _ in range(n)] for i in range(64)}
    dlog = {"G_%d" % i: g[i] for i in range(64)}
    if tpc == 2:
        secrets_int.update({"y_%d" % i: [r() for _ in range(n)] for i in range(64)})
        dlog["H"] = h
    for i in range(64):
        dlog["Q_%d" % i] = [(secrets_int["x_%d" % i][j] * g[i] + (secrets_int["y_%d" % i][j] * h if tpc == 2 else 0)) % L for j in range(n)]
    return (shape,) + _materialise(shape, n, secrets_int, dlog)


# ---- the same flows with the verdicts as an input (tests/degenerate_cases.py) ---------------------------------------------------------------
# _check_all_flows above asserts "every proof is accepted" and flips one response.  Degenerate inputs (an identity left-hand side, a
# commitment that is the identity) are refused by the reference, so here the oracle says what each verifier must answer, proof by proof.
class OracleExpectation:
    """What oracle/c answers for one batch: the proofs (chal [n][32], resp [n][m][32], coms [n][nc][32]), the per-proof verdicts of
    verify_compact (vc) and verify_batchable (vb), the verdict of one batch verification over all n (rc_batch) with its operand scalars
    (coeffs; None for n > 512 or when the transcript protocol already refuses), and the verdicts of two batches in one call (rc_many:
    n ordinary proofs, then the n proofs of this batch).  entropy, w [nc][n][16], w2 [nc][2n][16] and the ordinary batch are kept for the callers."""


def oracle_expectation(shape, n, secrets, inst, common, seed, ordinary, same_entropy=False, tl=b"degenerate", many=True):
    _, cst = shape.build()
    rng = np.random.default_rng(seed)
    E = OracleExpectation()
    E.tl, E.n = tl, n
    E.entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if same_entropy:
        E.entropy[:] = E.entropy[0]
    nc, m = len(shape.cons), len(shape.secret_names)
    E.w = rng.integers(0, 256, size=(nc, n, 16), dtype=np.uint8)
    E.w_each = np.ascontiguousarray(E.w.transpose(1, 0, 2))
    inst_names = [p for p, c in shape.points if not c]
    common_names = [p for p, c in shape.points if c]

    def pts(ins, j):
        return np.stack([common[common_names.index(p)] if c else ins[inst_names.index(p)][j] for p, c in shape.points])

    E.chal, E.resp, E.coms = np.zeros((n, 32), np.uint8), np.zeros((n, m, 32), np.uint8), np.zeros((n, nc, 32), np.uint8)
    E.vc, E.vb = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for j in range(n):
        p = pts(inst, j)
        E.chal[j], E.resp[j], E.coms[j], _ = C.prove(cst, tl, secrets[j], p, E.entropy[j].tobytes())
        E.vc[j] = C.verify_compact(cst, tl, p, E.chal[j], E.resp[j]) != 0
        E.vb[j] = C.verify_batchable(cst, tl, p, E.coms[j], E.resp[j], E.w_each[j]) != 0
    E.rc_batch = int(C.batch_verify(cst, tl, n, inst, common, E.coms, E.resp, E.w) != 0)
    E.coeffs = None
    if n <= 512:
        rc, osc, _ = C.batch_verify(cst, tl, n, inst, common, E.coms, E.resp, E.w, want_msm_inputs=True)
        if rc == 0:
            E.coeffs = osc
    E.rc_many = None
    if many:
        # batch 0: ordinary proofs (the oracle's, over the same common points), batch 1: this batch
        osec, oinst = ordinary
        k = len(osec)
        oe = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        op = [C.prove(cst, tl, osec[i], pts(oinst, i), oe[i].tobytes()) for i in range(k)]
        sel = np.arange(n) % k
        E.inst2 = np.ascontiguousarray(np.concatenate([oinst[:, sel], inst], axis=1))
        E.coms2 = np.ascontiguousarray(np.concatenate([np.stack([op[i][2] for i in sel]), E.coms]))
        E.resp2 = np.ascontiguousarray(np.concatenate([np.stack([op[i][1] for i in sel]), E.resp]))
        E.w2 = np.ascontiguousarray(np.concatenate([rng.integers(0, 256, size=(nc, n, 16), dtype=np.uint8), E.w], axis=1))
        E.rc_many = [int(C.batch_verify(cst, tl, n, np.ascontiguousarray(E.inst2[:, b * n:(b + 1) * n]), common, E.coms2[b * n:(b + 1) * n],
                                        E.resp2[b * n:(b + 1) * n], np.ascontiguousarray(E.w2[:, b * n:(b + 1) * n])) != 0) for b in range(2)]
    return E


def _first_diff(got, want):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    return None if len(bad) == 0 else int(bad[0])


def _check_flows_vs_oracle(eng, shape, n, secrets, inst, common, E, routes=(("host", NEVER), ("fused", 0)), names=None):
    """prove / verify_compact / verify_batchable (per proof) / batch_verify (with its operand scalars) / batch_verify_many on every route,
    against E (oracle_expectation): proofs byte for byte, verdicts proof by proof and batch by batch.  names: {index: text} for messages."""
    st, _ = shape.build()
    names = names or {}
    tl = E.tl
    what = lambda j: "proof %d (%s)" % (j, names.get(j, "ordinary"))
    out = {}
    for route, thr in routes:
        T.set_fused_min_batch(thr)
        try:
            ts = _fresh(tl, n)
            chal, resp, coms = T.prove_batch(eng, st, ts, secrets, inst, common, E.entropy)
            ts2 = _fresh(tl, n)
            res = T.verify_compact_batch(eng, st, ts2, inst, common, E.chal, E.resp)
            ok, coeffs = T.batch_verify_coeffs(eng, st, _fresh(tl, n), inst, common, E.coms, E.resp, E.w)
            ts4 = _fresh(tl, n)
            each = T.verify_batchable_each(eng, st, ts4, inst, common, E.coms, E.resp, E.w_each)
            verd = None
            if E.rc_many is not None:
                verd = T.batch_verify_many(eng, st, 2, _fresh(tl, 2 * n), E.inst2, common, E.coms2, E.resp2, E.w2)
            try:
                T.batch_verify(eng, st, _fresh(tl, n), inst, common, E.coms, E.resp, E.w)
                rc = 0
            except T.VerificationFailure:
                rc = 1
        finally:
            T.set_fused_min_batch(32)
        for name, got, want in (("challenge", chal, E.chal), ("responses", resp, E.resp), ("commitments", coms, E.coms)):
            j = _first_diff(got, want)
            assert j is None, "%s route: %s of %s differ from the oracle's prover" % (route, name, what(j))
        j = _first_diff(res, E.vc)
        assert j is None, "%s route: verify_compact says %d for %s, the oracle %d" % (route, res[j], what(j), E.vc[j])
        j = _first_diff(each, E.vb)
        assert j is None, "%s route: verify_batchable says %d for %s, the oracle %d" % (route, each[j], what(j), E.vb[j])
        assert rc == E.rc_batch and ok == (E.rc_batch == 0), "%s route: batch_verify %d / %r, the oracle %d" % (route, rc, ok, E.rc_batch)
        if E.coeffs is not None:
            j = _first_diff(coeffs, E.coeffs)
            assert j is None, "%s route: operand scalar %d of the batch verifier differs from the oracle's" % (route, j)
        if verd is not None:
            assert verd.tolist() == E.rc_many, "%s route: batch_verify_many %r, the oracle %r" % (route, verd.tolist(), E.rc_many)
        acc, acc_b = E.vc == 0, E.vb == 0
        out[route] = (chal, resp, coms, ts[:, :203], ts2[acc][:, :203], ts4[acc_b][:, :203])
    first = routes[0][0]
    for route, _ in routes[1:]:
        for a, b in zip(out[first], out[route]):
            assert a.shape == b.shape and (a == b).all(), "%s and %s routes leave different bytes" % (first, route)
    return out[routes[-1][0]]


# ---- the _dev entry points on device buffers (tests/test_gpu_degenerate.py: CMZ; tests/test_gpu_random_statements.py: any shape) ----------------
def fused_statement_of(shape):
    """the shape as zkp_amd.engine.FusedStatement: every secret allocated before the first point, the points in the shape's order"""
    from zkp_amd import engine as EN
    si = {s: i for i, s in enumerate(shape.secret_names)}
    pi = {p: i for i, (p, _) in enumerate(shape.points)}
    return EN.FusedStatement(shape.label, [s.encode() for s in shape.secret_names], [(p.encode(), c) for p, c in shape.points],
                             [(pi[lhs], [(si[s], pi[p]) for s, p in lc]) for lhs, lc in shape.cons])


def _torch():
    import torch
    assert torch.cuda.is_available(), "torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)"
    return torch


def dev_flows(e, fst, b, E, names=None, register=True, prove=True, after=None):
    """zkp_fused_prove_dev / _verify_compact_dev / _verify_batchable_dev / _batch_verify_dev on device buffers against E (oracle_expectation, with
    E.sub = (k, inst, coms, resp, w) of the proofs the oracle accepts one by one and E.rc_sub = its verdict on that batch).
    b: shape, n, secrets, inst, common.  fst = None: built from b.shape.  names: {index: text} for messages.  register = False: the common points
    are not registered for fixed-base tables.  prove = False: the verifiers only (E holds proofs the prover would not emit).
    after(call name): called when each entry point has finished, e.g. to read the engine's last_schedule()."""
    torch = _torch()
    fst = fst or fused_statement_of(b.shape)
    names = names or {}
    after = after or (lambda what: None)
    n, m, nc = b.n, len(b.shape.secret_names), len(b.shape.cons)
    ns, ni = len(b.common), len(b.inst)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
    t0 = T.Transcript(E.tl).state
    pos = int(t0[200]) | int(t0[201]) << 8 | int(t0[202]) << 16
    ts0 = np.stack([t0] * n)
    if register and len(b.common):
        e.prepare_fixed_points(b.common)
    table = np.concatenate([b.common, b.inst.reshape(-1, 32)])
    d_tbl = dev(table)
    if prove:
        d_ts, d_sec, d_ent = dev(ts0), dev(b.secrets), dev(E.entropy)
        d_chal, d_resp, d_coms, d_st = z(n, 32), z(n, m, 32), z(n, nc, 32), z(nc * n)
        torch.cuda.synchronize()
        e.fused_prove_dev(fst, n, pos, d_ts.data_ptr(), d_sec.data_ptr(), d_tbl.data_ptr(), d_ent.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(),
                          d_coms.data_ptr(), d_st.data_ptr())
        e.synchronize()
        after("prove")
        assert not d_st.cpu().numpy().any()
        for what, got, want in (("challenge", d_chal, E.chal), ("responses", d_resp, E.resp), ("commitments", d_coms, E.coms)):
            j = _first_diff(got.cpu().numpy(), want)
            assert j is None, "%s of proof %d (%s) differ from the oracle's prover" % (what, j, names.get(j, "ordinary"))
    # the verifiers on the ORACLE's proofs (equal to the device's by the lines above)
    d_chal, d_resp, d_coms = dev(E.chal), dev(E.resp), dev(E.coms)
    d_ts2, d_res = dev(ts0), z(n) + 7
    torch.cuda.synchronize()
    e.fused_verify_compact_dev(fst, n, pos, d_ts2.data_ptr(), d_tbl.data_ptr(), d_chal.data_ptr(), d_resp.data_ptr(), d_res.data_ptr())
    e.synchronize()
    after("verify_compact")
    j = _first_diff(d_res.cpu().numpy(), E.vc)
    assert j is None, "verify_compact_dev says %d for proof %d (%s), the oracle %d" % (d_res.cpu().numpy()[j], j, names.get(j, "ordinary"), E.vc[j])
    d_tbl_each = torch.cat([d_tbl, d_coms.reshape(-1, 32)])
    d_ts4, d_we, d_res4 = dev(ts0), dev(E.w_each), z(n) + 7
    torch.cuda.synchronize()
    e.fused_verify_batchable_dev(fst, n, pos, d_ts4.data_ptr(), d_tbl_each.data_ptr(), d_resp.data_ptr(), d_we.data_ptr(), d_res4.data_ptr())
    e.synchronize()
    after("verify_batchable")
    j = _first_diff(d_res4.cpu().numpy(), E.vb)
    assert j is None, "verify_batchable_dev says %d for proof %d (%s), the oracle %d" % (d_res4.cpu().numpy()[j], j, names.get(j, "ordinary"), E.vb[j])
    # one batch verification over all n, and one over the proofs the oracle accepts one by one
    for k, inst, coms, resp, w, want in ((n, b.inst, E.coms, E.resp, E.w, E.rc_batch),) + ((E.sub + (E.rc_sub,),) if E.sub[0] != n else ()):
        d_pts = z(ns + (ni + nc) * k, 32)
        d_pts[: ns + ni * k] = dev(np.concatenate([b.common, inst.reshape(-1, 32)]))
        d_ts3, d_c, d_r, d_w, d_out = dev(ts0[:k]), dev(coms), dev(resp), dev(w), z(32) + 1
        d_bst = torch.ones(2, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        e.fused_batch_verify_dev(fst, k, pos, d_ts3.data_ptr(), d_pts.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), d_w.data_ptr(), d_out.data_ptr(), d_bst.data_ptr())
        e.synchronize()
        after("batch_verify")
        got = int(d_out.cpu().numpy().any() or d_bst.cpu().numpy().any())
        assert got == want, "batch_verify_dev over %d proofs: %d, the oracle %d" % (k, got, want)

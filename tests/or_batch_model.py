"""The batchable 1-of-k OR-proof of include/zkp_or_batch_mi355x.h in plain Python over oracle.model: the prover that returns its
commitments, the exact per-proof verifier (decode the given commitment, compare points), the batch verifier's coefficient vector in Python
integers and its group check with M.msm_points.  Statements, inst and common are as in tests/or_proof_model.py; a proof is
(commitments [k][nc], challenges [k], responses [k][m]) of 32-byte strings."""
from oracle import model as M
from tests import or_proof_model as OM

L = M.L


def _point_ids(stmt):
    """allocation index -> point id (common points 0 .. ns - 1 by rank, instance points ns + rank), and (ns, ni)"""
    ranks = OM._ranks(stmt[2])
    ns = sum(1 for kind, _ in ranks if kind == "c")
    return [r if kind == "c" else ns + r for kind, r in ranks], ns, len(ranks) - ns


def prove(t, stmt, k, secrets, real, inst, common, entropy):
    """-> (commitments, challenges, responses), t advanced exactly as OM.prove advances it; None when a point does not decode"""
    _, names, points, constraints = stmt
    m, ranks = len(names), OM._ranks(points)
    OM._bind(t, stmt, k, inst, common, validate=False)
    rng = t.build_rng()
    for x in secrets:
        rng = rng.rekey_with_witness_bytes(b"", x)
    rng = rng.rekey_with_witness_bytes(b"", real.to_bytes(32, "little")).finalize(entropy)
    blind = [rng.random_scalar() for _ in range(m)]
    cs, ss = [], []
    for b in range(k):
        cs.append(rng.random_scalar())
        ss.append([rng.random_scalar() for _ in range(m)])
    C = [0 if b == real else cs[b] for b in range(k)]
    S = [blind if b == real else ss[b] for b in range(k)]
    coms = []
    for b in range(k):
        row = []
        for lhs, lc in constraints:
            ps = [_decode(ranks, v, inst[b], common) for _, v in lc] + [_decode(ranks, lhs, inst[b], common)]
            if any(p is None for p in ps):
                return None
            row.append(t.append_blinding_commitment(points[lhs][0], M.msm_points([S[b][s] for s, _ in lc] + [(L - C[b]) % L], ps)))
        coms.append(row)
    c = t.get_challenge(b"chal")
    c_real = (c - sum(C)) % L
    xs = [int.from_bytes(x, "little") % L for x in secrets]
    chal = [c_real if b == real else cs[b] for b in range(k)]
    resp = [[(blind[i] + c_real * xs[i]) % L for i in range(m)] if b == real else ss[b] for b in range(k)]
    return coms, [M.sc_to_bytes(x) for x in chal], [[M.sc_to_bytes(x) for x in row] for row in resp]


def _decode(ranks, v, inst_b, common):
    kind, r = ranks[v]
    return M.ristretto_decode(common[r] if kind == "c" else inst_b[r])


def exact_part(t, stmt, k, inst, common, coms, challenges, responses) -> bool:
    """steps 1 - 5 and the scalar check of step 6: what the batch verifier runs per proof.  t advances"""
    points, constraints = stmt[2], stmt[3]
    try:
        OM._bind(t, stmt, k, inst, common, validate=True)
    except OM.Rejected:
        return False
    ch = [int.from_bytes(x, "little") for x in challenges]
    if any(x >= L for x in ch) or any(int.from_bytes(x, "little") >= L for row in responses for x in row):
        return False
    try:
        for b in range(k):
            for (lhs, _), enc in zip(constraints, coms[b]):
                t.validate_and_append_blinding_commitment(points[lhs][0], enc)
    except M.VerificationFailure:
        return False
    return sum(ch) % L == t.get_challenge(b"chal")


def verify_batchable(t, stmt, k, inst, common, coms, challenges, responses) -> bool:
    if not exact_part(t, stmt, k, inst, common, coms, challenges, responses):
        return False
    ranks = OM._ranks(stmt[2])
    for b in range(k):
        cb = int.from_bytes(challenges[b], "little")
        rs = [int.from_bytes(x, "little") for x in responses[b]]
        for (lhs, lc), enc in zip(stmt[3], coms[b]):
            ps = [_decode(ranks, v, inst[b], common) for _, v in lc] + [_decode(ranks, lhs, inst[b], common)]
            given = M.ristretto_decode(enc)
            if given is None or any(p is None for p in ps):
                return False
            if M.ristretto_encode(M.msm_points([rs[s] for s, _ in lc] + [(L - cb) % L], ps)) != M.ristretto_encode(given):
                return False
    return True


def batch_coeffs(stmt, k, n, chal, resp, weights):
    """The coefficient vector over [common by point id (ns) | inst[b][v][j] (k ni n) | commitments [n][k][nc]] as Python integers mod l.
    chal[j][b], resp[j][b][i], weights[j][b][c]: integers"""
    pid, ns, ni = _point_ids(stmt)
    constraints = stmt[3]
    nc = len(constraints)
    out = [0] * (ns + n * k * (ni + nc))
    for j in range(n):
        for b in range(k):
            for c, (lhs, lc) in enumerate(constraints):
                r = weights[j][b][c]
                out[ns + k * ni * n + (j * k + b) * nc + c] = (L - r) % L
                for p, value in [(pid[v], resp[j][b][s]) for s, v in lc] + [(pid[lhs], -chal[j][b])]:
                    at = p if p < ns else ns + (b * ni + (p - ns)) * n + j
                    out[at] = (out[at] + r * value) % L
    return out


def batch_verify(ts, stmt, k, inst, common, coms, chal, resp, weights) -> bool:
    """ts: n model transcripts (advanced); inst[j][b][v], common[p], coms[j][b][c], chal[j][b], resp[j][b][i]: 32-byte strings"""
    n = len(ts)
    ok = True
    for j in range(n):
        ok &= exact_part(ts[j], stmt, k, inst[j], common, coms[j], chal[j], resp[j])
    if not ok:
        return False
    _, ns, ni = _point_ids(stmt)
    to_int = lambda x: int.from_bytes(x, "little")                      # noqa: E731
    coeffs = batch_coeffs(stmt, k, n, [[to_int(x) for x in row] for row in chal], [[[to_int(x) for x in r] for r in row] for row in resp], weights)
    encs = list(common) + [inst[j][b][v] for b in range(k) for v in range(ni) for j in range(n)] + [e for pj in coms for row in pj for e in row]
    pts = [M.ristretto_decode(e) for e in encs]
    if any(p is None for p in pts):
        return False
    return M.ristretto_encode(M.msm_points(coeffs, pts)) == M.IDENTITY_ENC

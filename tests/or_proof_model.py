"""The 1-of-k OR-proof of include/zkp_or_mi355x.h in plain Python over oracle.model: the reference the tests compare bytes with.

A statement is (label, secrets, points, constraints) as zkp_amd.toolbox.Statement keeps them: points = [(name, is_common)] in allocation
order, constraints = [(lhs, [(secret, point)])] with indices into those lists.  inst[b] holds the encodings of branch b's instance points in
allocation order, common the common points' in allocation order.  About 10 ms per proof at k = 3."""
from oracle import model as M

L = M.L


class Rejected(Exception):
    pass


def _ranks(points):
    """allocation index -> ("c" | "i", rank)"""
    out, nc, ni = [], 0, 0
    for _, common in points:
        if common:
            out.append(("c", nc)); nc += 1
        else:
            out.append(("i", ni)); ni += 1
    return out


def _bind(t, stmt, k, inst, common, validate):
    label, secrets, points, _ = stmt
    ranks = _ranks(points)
    t.domain_sep(label)
    t.append_message(b"or-branches", k.to_bytes(4, "little"))
    for name in secrets:
        t.append_scalar_var(name)

    def put(name, enc):
        if validate and enc == M.IDENTITY_ENC:
            raise Rejected()
        t.append_message(b"ptvar", name)
        t.append_message(b"val", enc)

    for b in range(k):
        for (name, _), (kind, r) in zip(points, ranks):
            if kind == "i":
                put(name, inst[b][r])
    for (name, _), (kind, r) in zip(points, ranks):
        if kind == "c":
            put(name, common[r])


def _commitments(t, stmt, k, inst, common, S, C):
    """com[b][c] = sum_t S[b][sec] P_b[pt] + (l - C[b]) P_b[lhs], appended in order; None if a point does not decode"""
    _, _, points, constraints = stmt
    ranks = _ranks(points)
    ok = True
    for b in range(k):
        def point(v):
            kind, r = ranks[v]
            return M.ristretto_decode(common[r] if kind == "c" else inst[b][r])
        for lhs, lc in constraints:
            ps = [point(v) for _, v in lc] + [point(lhs)]
            if any(p is None for p in ps):
                ok = False
                continue
            com = M.msm_points([S[b][s] for s, _ in lc] + [(L - C[b]) % L], ps)
            t.append_blinding_commitment(points[lhs][0], com)
    return ok


def prove(t, stmt, k, secrets, real, inst, common, entropy):
    """-> (challenges [k] of 32 bytes, responses [k][m] of 32 bytes), t advanced; None when a point does not decode"""
    m = len(stmt[1])
    _bind(t, stmt, k, inst, common, validate=False)
    rng = t.build_rng()
    for x in secrets:
        rng = rng.rekey_with_witness_bytes(b"", x)
    rng = rng.rekey_with_witness_bytes(b"", real.to_bytes(32, "little"))
    rng = rng.finalize(entropy)
    blind = [rng.random_scalar() for _ in range(m)]
    cs, ss = [], []
    for b in range(k):
        cs.append(rng.random_scalar())
        ss.append([rng.random_scalar() for _ in range(m)])
    C = [0 if b == real else cs[b] for b in range(k)]
    S = [blind if b == real else ss[b] for b in range(k)]
    if not _commitments(t, stmt, k, inst, common, S, C):
        return None
    c = t.get_challenge(b"chal")
    c_real = (c - sum(C)) % L
    xs = [int.from_bytes(x, "little") % L for x in secrets]
    chal = [c_real if b == real else cs[b] for b in range(k)]
    resp = [[(blind[i] + c_real * xs[i]) % L for i in range(m)] if b == real else ss[b] for b in range(k)]
    return [M.sc_to_bytes(x) for x in chal], [[M.sc_to_bytes(x) for x in row] for row in resp]


def verify(t, stmt, k, inst, common, challenges, responses) -> bool:
    try:
        _bind(t, stmt, k, inst, common, validate=True)
    except Rejected:
        return False
    ch = [int.from_bytes(x, "little") for x in challenges]
    rs = [[int.from_bytes(x, "little") for x in row] for row in responses]
    if any(x >= L for x in ch) or any(x >= L for row in rs for x in row):
        return False
    if not _commitments(t, stmt, k, inst, common, rs, ch):
        return False
    return sum(ch) % L == t.get_challenge(b"chal")

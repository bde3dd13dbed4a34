"""(helper module of tests/test_host_degenerate.py and tests/test_gpu_degenerate.py)
Degenerate witnesses and coinciding points, for every flow.  Every other flow test proves with uniform canonical witnesses and points in
general position (tests/statement_shapes.py: every point is d * B with an independent random d).  This table builds batches in which
chosen proofs are degenerate and the rest ordinary: witnesses 0, 1, l - 1, the sign-fold boundary, non-canonical 32-byte strings; two
point slots holding one element, a slot holding the negative of another, left-hand sides and honest commitments that are the identity.
Every point still has a known discrete log, so every left-hand side is computed here, with Python integers.

Nothing here says which proofs verify: tests/statement_shapes.py::_check_flows_vs_oracle asks the oracles.  What the oracles answered when
this table was written (mod.rs:186-221: validate_and_append_point_var refuses the identity): a proof with an identity instance point --
families neg_cancel and zero_secrets, every witness family whose value is 0 mod l in the slot (or in all slots) of a constraint whose
terms all vanish -- is refused by every verifier; everything else is accepted, non-canonical witnesses included.

The contract for a witness >= l (include/zkp_mi355x.h, prover.rs:80): the prover's RNG is re-keyed with the caller's 32 bytes as given;
the response is (s mod l) c + b mod l.  Witnesses are therefore raw 32-byte strings here and never pass through _sc (which reduces).
"""
import numpy as np

from oracle import model as M
from tests.statement_shapes import Shape, _mul_base, _shape_case

L = M.L
_Q = (2**256 - 1) // L

# ---- witness families: raw 256-bit values ---------------------------------------------------------------------------------------------
CANONICAL = [("0", 0), ("1", 1), ("2", 2), ("l-1", L - 1), ("l-2", L - 2), ("(l-1)/2", (L - 1) // 2), ("(l+1)/2", (L + 1) // 2),
             ("2^128-1", 2**128 - 1), ("2^128", 2**128), ("2^252-1", 2**252 - 1), ("2^252", 2**252)]
NON_CANONICAL = [("l", L), ("l+1", L + 1), ("2l-1", 2 * L - 1), ("2^253-1", 2**253 - 1), ("2^255", 2**255), ("ql-1", _Q * L - 1), ("ql", _Q * L),
                 ("2^256-1", 2**256 - 1)]                                   # q = floor((2^256 - 1) / l): ql is the largest multiple of l in 256 bits
assert all(v < L for _, v in CANONICAL) and all(L <= v < 2**256 for _, v in NON_CANONICAL)
WITNESS_VALUES = dict(CANONICAL + NON_CANONICAL)
WITNESS_FAMILIES = ["w:" + k for k, _ in CANONICAL + NON_CANONICAL]

# ---- point families -----------------------------------------------------------------------------------------------------------------------
# proof level: one proof of a batch is degenerate on its own; batch level: the property belongs to the common points or to the whole batch
POINT_FAMILIES_PROOF = ["inst_eq_inst", "inst_eq_common_tabled", "inst_eq_common_untabled", "neg_cancel", "zero_secrets", "x_is_one", "x_is_minus_one",
                        "small_multiples_instance"]
POINT_FAMILIES_BATCH = ["common_eq_common", "same_instance_points", "identical_proofs", "small_multiples_common"]
FAMILIES = WITNESS_FAMILIES + POINT_FAMILIES_PROOF + POINT_FAMILIES_BATCH
SMALL = [1, 2, 8, L - 1]                                                    # B, 2B, 8B, (l - 1)B = -B

PLACEMENT = (0, 31, 32, 63, 64, 255, 256)                                   # and n - 1: lane, wavefront and 32-proof ragged block edges


# ---- statements -------------------------------------------------------------------------------------------------------------------------------
def _cmz_shape():
    st = M.cmz_statement(10)
    return Shape(st.label, st.secrets, [(p, False) for p in st.instance] + [(p, True) for p in st.common], st.constraints)


def _gens70_shape():
    xs, gs = ["x_%d" % i for i in range(70)], ["G_%d" % i for i in range(70)]
    return Shape(b"W70", xs, [("Q", False)] + [(g, True) for g in gs], [("Q", [(x, g) for x, g in zip(xs, gs)])])


STATEMENTS = {
    # define_proof! {dleq, "DLEQ proof", (x), (A, B, H), (G) : A = (x * G), B = (x * H)}   (benches/zkp.rs:49)
    "dleq_macro": lambda: Shape(b"DLEQ proof", ["x"], [("A", False), ("B", False), ("H", False), ("G", True)], [("A", [("x", "G")]), ("B", [("x", "H")])]),
    # tests/dleq_using_constraint_api.rs:41-56: allocation order x, B, H, A, G; A = x B, G = x H; no common point
    "dleq_capi": lambda: Shape(b"DLEQProof", ["x"], [("B", False), ("H", False), ("A", False), ("G", False)], [("A", [("x", "B")]), ("G", [("x", "H")])]),
    "cmz10": _cmz_shape,                                                    # P in 10 of 11 constraints, Q once: paired terms and riders' tables
    "repeated_term": lambda: _shape_case("repeated_term", 1, np.random.default_rng(0))[0],
    "lhs_is_rhs_elsewhere": lambda: _shape_case("lhs_is_rhs_elsewhere", 1, np.random.default_rng(0))[0],
    "instance_lhs_twice": lambda: _shape_case("instance_lhs_twice", 1, np.random.default_rng(0))[0],
    # one secret times a point and times its negative in one constraint (family neg_cancel needs it; no statement above has such a constraint)
    "cancelling_pair": lambda: Shape(b"cancelling pair", ["x", "y"], [("A", False), ("P", False), ("N", False), ("K", False), ("G", True)],
                                     [("A", [("x", "P"), ("x", "N")]), ("K", [("y", "G")])]),
    # 70 common generators: 64 get fixed-base tables, six stay without (tests/test_gpu_toolbox.py: more common points than table slots)
    "gens70": _gens70_shape,
}

# (statement, family) -> why the family cannot be built for the statement.  Counted by a test of its own, so that a new statement or family
# must either get a recipe or a reason.
_ONE_INST = "the statement has one instance point"
_NO_FREE = "no instance point is free (each is a left-hand side): equality with a common point is reached through the witness, family x_is_one"
_ALL_TABLED = "every common point gets a fixed-base table (at most 64 common points)"
_ONE_COMMON = "fewer than two common points"
_NO_PAIR = "no constraint multiplies one secret into two point slots"
NOT_APPLICABLE = {
    ("repeated_term", "inst_eq_inst"): _ONE_INST, ("instance_lhs_twice", "inst_eq_inst"): _ONE_INST, ("gens70", "inst_eq_inst"): _ONE_INST,
    ("dleq_capi", "inst_eq_common_tabled"): "no common point", ("lhs_is_rhs_elsewhere", "inst_eq_common_tabled"): _NO_FREE,
    ("repeated_term", "inst_eq_common_tabled"): _NO_FREE, ("instance_lhs_twice", "inst_eq_common_tabled"): _NO_FREE,
    ("dleq_macro", "inst_eq_common_untabled"): _ALL_TABLED, ("dleq_capi", "inst_eq_common_untabled"): "no common point",
    ("cmz10", "inst_eq_common_untabled"): _ALL_TABLED, ("repeated_term", "inst_eq_common_untabled"): _ALL_TABLED,
    ("lhs_is_rhs_elsewhere", "inst_eq_common_untabled"): _ALL_TABLED, ("instance_lhs_twice", "inst_eq_common_untabled"): _ALL_TABLED,
    ("cancelling_pair", "inst_eq_common_untabled"): _ALL_TABLED,
    ("dleq_macro", "neg_cancel"): _NO_PAIR, ("dleq_capi", "neg_cancel"): _NO_PAIR, ("cmz10", "neg_cancel"): _NO_PAIR,
    ("repeated_term", "neg_cancel"): "x multiplies G twice, but G = -G has no solution in a group of odd order",
    ("lhs_is_rhs_elsewhere", "neg_cancel"): _NO_PAIR, ("instance_lhs_twice", "neg_cancel"): _NO_PAIR, ("gens70", "neg_cancel"): _NO_PAIR,
    ("repeated_term", "small_multiples_instance"): _NO_FREE, ("lhs_is_rhs_elsewhere", "small_multiples_instance"): _NO_FREE,
    ("instance_lhs_twice", "small_multiples_instance"): _NO_FREE, ("gens70", "small_multiples_instance"): _NO_FREE,
    ("dleq_macro", "common_eq_common"): _ONE_COMMON, ("dleq_capi", "common_eq_common"): _ONE_COMMON, ("repeated_term", "common_eq_common"): _ONE_COMMON,
    ("lhs_is_rhs_elsewhere", "common_eq_common"): _ONE_COMMON, ("cancelling_pair", "common_eq_common"): _ONE_COMMON,
    ("dleq_capi", "small_multiples_common"): "no common point",
}
# witness cases that cannot be built: instance_lhs_twice ties its two secrets (A = x G = y H, so y = x g / h); the same value in both slots
# needs G = H (family common_eq_common puts the two on one element) or a value that is 0 mod l
WITNESS_ALL_SLOTS_TIED = {"instance_lhs_twice": "x and y are tied by A = x G = y H: one value in both slots needs G = H"}


def applicable(stname, fam):
    return (stname, fam) not in NOT_APPLICABLE


def families_of(stname, level=None):
    fams = {"proof": WITNESS_FAMILIES + POINT_FAMILIES_PROOF, "batch": POINT_FAMILIES_BATCH, None: FAMILIES}[level]
    return [f for f in fams if applicable(stname, f)]


# ---- recipes: one proof ---------------------------------------------------------------------------------------------------------------------
def _set(sec, **kv):
    sec.update(kv)
    return set(kv)


def witness_cases(stname, shape):
    """the cases of a witness family: the value in each secret slot in turn, then in every slot at once"""
    return list(shape.secret_names) + ([] if stname in WITNESS_ALL_SLOTS_TIED else ["all"])


def _recipe(stname, fam, k, shape, sec, d, cd):
    """Makes the draft (sec: secret name -> raw 256-bit int, d: free instance point -> discrete log; cd: the common points' logs, read only)
    degenerate in the way `fam` says; k picks the case inside the family.  -> (description, names of the secrets it pinned)"""
    names = shape.secret_names
    if fam.startswith("w:"):
        v = WITNESS_VALUES[fam[2:]]
        cases = witness_cases(stname, shape)
        slot = cases[k % len(cases)]
        if slot == "all":
            for s in names:
                sec[s] = v
            return "%s in every slot" % fam[2:], set(names)
        sec[slot] = v
        return "%s in %s" % (fam[2:], slot), {slot}
    S = stname
    if fam == "inst_eq_inst":
        if S == "dleq_macro":
            d["H"] = cd["G"]                                            # H = G, hence A = B
            return "H = G, A = B", set()
        if S == "dleq_capi":
            d["H"] = d["B"]
            return "H = B, A = G", set()
        if S == "cmz10":
            d["Q"] = d["P"]
            return "Q = P", set()
        if S == "lhs_is_rhs_elsewhere":
            return "y = 0: B = A", _set(sec, y=0)
        if S == "cancelling_pair":
            d["N"] = d["P"]
            return "N = P", set()
    if fam == "inst_eq_common_tabled":
        if S == "dleq_macro":
            d["H"] = cd["G"]
            return "H = G", set()
        if S == "cmz10":
            d["P"] = cd["A"]                                            # both terms of C_i = m_i P + z_i A on one element
            return "P = A", set()
        if S == "cancelling_pair":
            d["P"] = cd["G"]
            return "P = G", set()
        if S == "gens70":
            for s in names:
                sec[s] = 0
            sec["x_0"] = 1
            return "Q = G_0 (tabled)", set(names)
    if fam == "inst_eq_common_untabled" and S == "gens70":
        for s in names:
            sec[s] = 0
        sec["x_69"] = 1
        return "Q = G_69 (no table)", set(names)
    if fam == "neg_cancel" and S == "cancelling_pair":
        d["N"] = (L - d["P"]) % L
        return "N = -P: A and its commitment are the identity", set()
    if fam in ("zero_secrets", "x_is_one", "x_is_minus_one"):
        v = {"zero_secrets": 0, "x_is_one": 1, "x_is_minus_one": L - 1}[fam]
        if S in ("dleq_macro", "dleq_capi", "lhs_is_rhs_elsewhere", "instance_lhs_twice"):
            return "x = %s" % fam, _set(sec, x=v)
        if S == "cmz10":
            return "m_1 = %s, z_1 = 0: C_1 from P alone" % fam, _set(sec, m_1=v, z_1=0)
        if S == "repeated_term":
            return "x = 0, y = %s: A from G alone" % fam, _set(sec, x=0, y=v)
        if S == "cancelling_pair":
            return "y = %s" % fam, _set(sec, y=v)
        if S == "gens70":
            for s in names:
                sec[s] = 0
            sec["x_%d" % (k % 70)] = v
            return "x_%d = %s, the rest 0" % (k % 70, fam), set(names)
    if fam == "small_multiples_instance":
        free = sorted(d)
        for i, p in enumerate(free):
            d[p] = SMALL[(k + i) % 4]
        return "free instance points " + ", ".join("%s = %s B" % (p, "(l-1)" if d[p] == L - 1 else d[p]) for p in free), set()
    raise KeyError((stname, fam))


def _tie(stname, sec, cd, pinned):
    """secrets that the statement ties to each other follow the pinned one"""
    if stname == "instance_lhs_twice":
        g, h = cd["G"], cd["H"]
        if "y" in pinned and "x" not in pinned:
            sec["x"] = sec["y"] % L * h * pow(g, -1, L) % L
        else:
            sec["y"] = sec["x"] % L * g * pow(h, -1, L) % L


def _solve(shape, sec, d, cd):
    """left-hand sides from the secrets (mod l) and the right-hand sides' logs, constraint by constraint"""
    common = dict(shape.points)
    d = dict(d)
    for lhs, lc in shape.cons:
        v = sum(sec[s] * (cd[p] if common[p] else d[p]) for s, p in lc) % L
        assert not common[lhs]
        if lhs in d:
            assert d[lhs] == v, (lhs, "the statement would be false")
        else:
            d[lhs] = v
    return d


class Batch:
    """shape, stname, n, secrets [n][m][32], inst [ni][n][32], common [ns][32], degenerate {index: (family, description)}, same_entropy,
    ordinary = (secrets [2][m][32], inst [ni][2][32]): two more ordinary proofs over the same common points"""


def _k_for(j, n, ncases):
    """case number of proof j: every case when the batch is large enough, else spread from the last case (all slots) down to the first"""
    if n >= ncases or n < 2:
        return j % ncases
    return (ncases - 1) - j * ((ncases - 1) // (n - 1))


def build_batch(stname, n, plan, seed, batch_family=None):
    """plan: {index: family} of proof-level families; batch_family: one of POINT_FAMILIES_BATCH or None"""
    shape = STATEMENTS[stname]()
    rng = np.random.default_rng(seed)
    r = lambda: int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1
    lhs_names = {lhs for lhs, _ in shape.cons}
    common_names = [p for p, c in shape.points if c]
    inst_names = [p for p, c in shape.points if not c]
    free = [p for p in inst_names if p not in lhs_names]
    cd = {p: r() for p in common_names}
    degenerate = {}
    if batch_family == "common_eq_common":
        if stname == "cmz10":
            cd["X_2"], cd["B"] = cd["X_1"], cd["A"]
        elif stname == "gens70":
            cd["G_1"] = cd["G_69"] = cd["G_0"]                          # a tabled and an untabled slot on G_0's element
        else:
            cd[common_names[1]] = cd[common_names[0]]
    elif batch_family == "small_multiples_common":
        for i, p in enumerate(common_names):
            cd[p] = SMALL[i % 4]
    secrets = np.zeros((n + 2, len(shape.secret_names), 32), np.uint8)
    dl = {p: [] for p in inst_names}
    whole = len(plan) == n
    for j in range(n + 2):
        sec = {s: r() for s in shape.secret_names}
        d = {p: r() for p in free}
        pinned = set()
        if j < n and j in plan:
            fam = plan[j]
            ncases = len(witness_cases(stname, shape)) if fam.startswith("w:") else max(4, len(shape.secret_names))
            desc, pinned = _recipe(stname, fam, _k_for(j, n, ncases) if whole else j + seed, shape, sec, d, cd)
            degenerate[j] = (fam, desc)
        _tie(stname, sec, cd, pinned)
        d = _solve(shape, sec, d, cd)
        for i, s in enumerate(shape.secret_names):
            secrets[j, i] = np.frombuffer(sec[s].to_bytes(32, "little"), np.uint8)          # raw: never reduced
        for p in inst_names:
            dl[p].append(d[p])
    common = _mul_base([cd[p] for p in common_names]) if common_names else np.zeros((0, 32), np.uint8)
    inst = np.stack([_mul_base(dl[p]) for p in inst_names])
    b = Batch()
    b.stname, b.shape, b.n, b.same_entropy = stname, shape, n, False
    b.ordinary = (secrets[n:].copy(), np.ascontiguousarray(inst[:, n:]))
    secrets, inst = secrets[:n].copy(), np.ascontiguousarray(inst[:, :n])
    if batch_family in ("same_instance_points", "identical_proofs"):
        # every proof of the batch carries the instance points (hence the witnesses) of proof 0; identical_proofs: the entropy too
        secrets[:] = secrets[0]
        inst[:] = inst[:, :1]
        b.same_entropy = batch_family == "identical_proofs"
    if batch_family is not None:
        degenerate = {j: (batch_family, batch_family) for j in range(n)}
    b.secrets, b.inst, b.common, b.degenerate = secrets, inst, np.ascontiguousarray(common), degenerate
    return b


def placement(n):
    return sorted({i for i in PLACEMENT if i < n} | {n - 1})


def mixed_plans(stname, n):
    """the proof-level families of a statement, one per placement index, in as many batches as that takes -> [{index: family}]"""
    fams, idx = families_of(stname, "proof"), placement(n)
    return [dict(zip(idx, fams[i:i + len(idx)])) for i in range(0, len(fams), len(idx))]


def dense_plan(stname, n):
    """every proof-level family of a statement in ONE batch: the first ones at the placement indices, the rest at every fifth index
    from 2 on, ordinary proofs between them -> {index: family}"""
    fams, idx = families_of(stname, "proof"), placement(n)
    rest = [i for i in range(2, n - 1, 5) if i not in idx]
    assert len(fams) <= len(idx) + len(rest), "n is too small for a dense plan"
    return dict(zip(idx + rest, fams))


def whole_batch(stname, fam, n, seed):
    """a batch in which every proof is degenerate in the way of one family"""
    if fam in POINT_FAMILIES_BATCH:
        return build_batch(stname, n, {}, seed, batch_family=fam)
    return build_batch(stname, n, {j: fam for j in range(n)}, seed)


def seed_of(*parts):
    return sum(sum(str(p).encode()) * (i + 1) for i, p in enumerate(parts))


def model_prove(shape, transcript, secrets32, points32, entropy32):
    """oracle/model.py's prover in the shape's allocation order, witnesses as raw bytes -> (challenge, responses [m][32], commitments [nc][32])"""
    pr = M.Prover(shape.label, transcript)
    sv = {s: pr.allocate_scalar(s.encode(), secrets32[i].tobytes()) for i, s in enumerate(shape.secret_names)}
    pv = {}
    for i, (p, _) in enumerate(shape.points):
        pv[p], _enc = pr.allocate_point(p.encode(), M.ristretto_decode(points32[i].tobytes()))
    for lhs, lc in shape.cons:
        pr.constrain(pv[lhs], [(sv[s], pv[p]) for s, p in lc])
    c, resp, coms, _ = pr._prove_impl(entropy32)
    tob = lambda v: np.frombuffer(M.sc_to_bytes(v), np.uint8)
    return tob(c), np.stack([tob(x) for x in resp]), np.stack([np.frombuffer(k_, np.uint8) for k_ in coms])


def model_verify_compact(shape, transcript, points32, chal, resp):
    """-> 0 accepted, 1 VerificationFailure (allocation of an identity point included: mod.rs:191-193)"""
    vr = M.Verifier(shape.label, transcript)
    try:
        sv = {s: vr.allocate_scalar(s.encode()) for s in shape.secret_names}
        pv = {p: vr.allocate_point(p.encode(), points32[i].tobytes()) for i, (p, _) in enumerate(shape.points)}
        for lhs, lc in shape.cons:
            vr.constrain(pv[lhs], [(sv[s], pv[p]) for s, p in lc])
        ints = lambda a: int.from_bytes(a.tobytes(), "little")
        vr.verify_compact(M.CompactProof(ints(chal), [ints(x) for x in resp]))
    except M.VerificationFailure:
        return 1
    return 0


def points_of(batch, j, inst=None):
    """the points of proof j in allocation order [np][32] (what the oracle's per-proof calls take)"""
    shape = batch.shape
    inst = batch.inst if inst is None else inst
    inst_names = [p for p, c in shape.points if not c]
    common_names = [p for p, c in shape.points if c]
    return np.stack([batch.common[common_names.index(p)] if c else inst[inst_names.index(p)][j] for p, c in shape.points])

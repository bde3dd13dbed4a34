"""(helper module of tests/test_host_random_statements.py and tests/test_gpu_random_statements.py)
A seeded generator of TRUE statements on top of tests/statement_shapes.py, for the four pieces of code that decide from a statement's shape
alone how every term of a batch is computed: pair_terms (csrc/stmt_pairs.h), cfg_from_terms / pick_teeth (csrc/fused_flows.h,
zkp_kernels.hip), k_stmt_classify (csrc/hot_tables.h) and the walks that act on their lists.

FAMILIES: named, deterministic statements, each built for one state of those rules that CMZ and the hand-written shapes never reach.
random_statement(seed): 0-6 common points, 1-12 instance points, 1-8 constraints of 1-12 terms, point ids drawn with a skew so that
use counts from 1 to 12 all occur.  census(shape, flow): what the plan must derive for the prover's and the verifier's job, restated
in plain Python from the comments of those headers (the pairs themselves come from t_pair_terms of tests/host/tr_host_lib.cpp, whose
rule tests/test_host_stmt_pairs.py checks).

Every point is d * B for a known d.  The constraints are processed in order: a left-hand side that is not yet determined is defined
by its constraint; one that is (a second constraint on it, or a common point) is reconciled by solving for a secret that only this
constraint uses; a left-hand side never appears on an earlier or its own right-hand side."""
import collections

import numpy as np

from oracle import cbind as C
from zkp_amd import toolbox as T
from tests import statement_shapes as SH
from tests.statement_shapes import L, NEVER, Shape, _materialise, oracle_expectation, _check_flows_vs_oracle, _first_diff, _fresh

UNPAIRED, ABSORBED = 0xFFFFFFFF, 0x80000000
STMT_RIDER_MIN = 2            # stmt_pairs.h: a per-proof point ALL of whose terms ride gets a table of multiples from this many riders on
GROUP_MIN_USES = 10           # hot_tables.h: from this many cold uses on, a point's terms are listed together (constant-time calls, 16 teeth)
NO_GROUPS = 0xFFFFFFFF
STMT_MIN_TERMS = 1024         # zkp_kernels.hip: stmt_classify_applies -- the one-launch classifier runs from this many terms on
N_SMALL = 6
SEEDS = (0, 1, 2, 3, 4, 5, 6, 10, 17, 25, 52, 107)      # the random statements the GPU tests run; 0, 10, 17, 25, 52, 107 reach every edge of RANDOM_EDGES between them


# ---- building statements ------------------------------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, label):
        self.label, self.secrets, self.points, self.cons = label, [], [], []

    def pts(self, names, common=False):
        names = names.split() if isinstance(names, str) else list(names)
        self.points += [(p, common) for p in names]
        return names

    def sec(self, name=None):
        name = name or "s%d" % len(self.secrets)
        self.secrets.append(name)
        return name

    def con(self, lhs, points, secrets=None):
        """lhs = sum s_i * P_i; a fresh secret per term unless named"""
        self.cons.append((lhs, [((secrets[i] if secrets and secrets[i] else self.sec()), p) for i, p in enumerate(points)]))

    def shape(self):
        return Shape(self.label, self.secrets, self.points, self.cons)


def _rider_at_min():
    # C1 = a P + x G ; C2 = b P + y G: the single-use C1, C2 each carry a term of P -> P: cnt 0, acnt 2 = STMT_RIDER_MIN
    b = _Builder(b"rider at min")
    b.pts("G", True), b.pts("P C1 C2")
    b.con("C1", ["P", "G"]), b.con("C2", ["P", "G"])
    return b.shape()


def _rider_below_min():
    # C1 = a P + x G ; D = y G: P (one use) carries C1 -> C1: cnt 0, acnt 1: on no class list, no table, the rider builds its own multiples
    b = _Builder(b"rider below min")
    b.pts("G", True), b.pts("P C1 D")
    b.con("C1", ["P", "G"]), b.con("D", ["G"])
    return b.shape()


def _partial_rider_leaves_one_use():
    # C1 = a P + x G ; D = b P + y G ; D = z H: P has two uses, the one next to C1 rides, the one next to D (two uses) stays -> P: cnt 1, acnt 1
    b = _Builder(b"partial rider, one use left")
    b.pts("G H", True), b.pts("P C1 D")
    b.con("C1", ["P", "G"]), b.con("D", ["P", "G"]), b.con("D", ["H"])
    return b.shape()


def _partial_rider_leaves_two_uses():
    # ... and with D = c P + z H: P: cnt 2, acnt 1 (a comb table for two of three terms)
    b = _Builder(b"partial rider, two uses left")
    b.pts("G H", True), b.pts("P C1 D")
    b.con("C1", ["P", "G"]), b.con("D", ["P", "G"]), b.con("D", ["P", "H"])
    return b.shape()


def _three_singles_one_constraint():
    # C = a P + b Q + x G with P, Q, C of one use each: P carries Q, C stays alone
    b = _Builder(b"three singles")
    b.pts("G", True), b.pts("P Q C")
    b.con("C", ["P", "Q", "G"])
    return b.shape()


def _lhs_rides_elsewhere():
    # A = x G = y H ; B = z A + w G: A is left-hand side twice and rides on B's chain in a third constraint (cnt 2, acnt 1)
    # A2 = u G ; B2 = v A2: a left-hand side that is another constraint's only right-hand side term (cnt 1, acnt 1)
    b = _Builder(b"lhs rides elsewhere")
    b.pts("G H", True), b.pts("A B A2 B2")
    b.con("A", ["G"]), b.con("A", ["H"]), b.con("B", ["A", "G"]), b.con("A2", ["G"]), b.con("B2", ["A2"])
    return b.shape()


def _group_edges_9_10_11():
    # eleven constraints C_i = a_i P11 + b_i P10 (i < 10) + c_i P9 (i < 9) + x_i G: 11, 10 and 9 prover-side uses around GROUP_MIN_USES
    b = _Builder(b"group edges")
    b.pts("G", True), b.pts("P11 P10 P9"), b.pts(["C%d" % i for i in range(11)])
    for i in range(11):
        b.con("C%d" % i, ["P11"] + (["P10"] if i < 10 else []) + (["P9"] if i < 9 else []) + ["G"])
    return b.shape()


MANY_GROUPS_USES = (10, 11, 12, 13, 10, 13)


def _many_groups_mixed_sizes():
    # six per-proof points with 10 .. 13 prover-side uses: a wavefront of the grouped walk spans several points of different sizes
    b = _Builder(b"many groups")
    b.pts("G", True), b.pts(["P%d" % j for j in range(6)]), b.pts(["C%d" % i for i in range(13)])
    for i in range(13):
        b.con("C%d" % i, ["P%d" % j for j, u in enumerate(MANY_GROUPS_USES) if i < u] + ["G"])
    return b.shape()


def _four_teeth_with_pairs():
    # no common point, every point of one use: no table anywhere (pick_teeth -> 4) while terms pair in every constraint
    b = _Builder(b"four teeth with pairs")
    b.pts("P Q R S U V C1 C2 A")
    b.con("C1", ["P", "Q"]), b.con("C2", ["R"]), b.con("A", ["S", "U", "V"])
    return b.shape()


UNEVEN_LENGTHS = (2, 33, 1, 31, 7)


def _uneven_constraint_lengths():
    # constraints of 2, 33, 1, 31 and 7 terms (not in descending order: d_order has to sort them) over four common and six per-proof points
    b = _Builder(b"uneven lengths")
    pool = b.pts("G0 G1 G2 G3", True) + b.pts("Q0 Q1 Q2 Q3 Q4 Q5")
    b.pts(["C%d" % k for k in range(5)])
    for k, n in enumerate(UNEVEN_LENGTHS):
        b.con("C%d" % k, [pool[(3 * t + k) % len(pool)] for t in range(n)])
    return b.shape()


def _static_uses_at_group_edge():
    # 27 constraints of 13 terms over 117 common points with exactly three uses each: 351 terms per proof, so three proofs already take the
    # one-launch classifier, where an unregistered common point has 3 N cold uses: 9 at N = 3 (a comb table), 12 at N = 4 (a group)
    b = _Builder(b"static uses at group edge")
    g = b.pts(["G%d" % i for i in range(117)], True)
    b.pts(["C%d" % k for k in range(27)])
    for k in range(27):
        b.con("C%d" % k, [g[(13 * k + t) % 117] for t in range(13)])
    return b.shape()


def _kitchen_sink():
    # unreferenced instance and common points (W, U0), a secret in no constraint (idle), one secret in several point slots (x on P, G, Q, H),
    # a repeated term on a multi-use point ((y, P) twice)
    b = _Builder(b"kitchen sink")
    x, idle, y, z = b.sec("x"), b.sec("idle"), b.sec("y"), b.sec("z")
    b.pts("G", True), b.pts("P W"), b.pts("U0 H", True), b.pts("Q C1 C2 C3")
    b.con("C1", ["P", "G", "P", "P"], [x, x, y, y])
    b.con("C2", ["Q", "H", "P"], [x, z, y])
    b.con("C3", ["G", "H"], [z, x])
    return b.shape()


FAMILIES = collections.OrderedDict([
    ("rider_at_min", _rider_at_min), ("rider_below_min", _rider_below_min), ("partial_rider_leaves_one_use", _partial_rider_leaves_one_use),
    ("partial_rider_leaves_two_uses", _partial_rider_leaves_two_uses), ("three_singles_one_constraint", _three_singles_one_constraint),
    ("lhs_rides_elsewhere", _lhs_rides_elsewhere), ("group_edges_9_10_11", _group_edges_9_10_11), ("many_groups_mixed_sizes", _many_groups_mixed_sizes),
    ("four_teeth_with_pairs", _four_teeth_with_pairs), ("uneven_constraint_lengths", _uneven_constraint_lengths),
    ("static_uses_at_group_edge", _static_uses_at_group_edge), ("kitchen_sink", _kitchen_sink)])


def random_statement(seed):
    """0-6 common points, 1-12 instance points, 1-8 constraints of 1-12 terms.  (A statement of one point gets a common point: a constraint needs
    a point besides its left-hand side.  A statement whose points have all been used on right-hand sides takes no further constraint.)"""
    rng = np.random.default_rng([int(seed), 0x57A7])
    ns, ni, ncons = int(rng.integers(0, 7)), int(rng.integers(1, 13)), int(rng.integers(1, 9))
    if ns + ni < 2:
        ns = 1
    kinds = [True] * ns + [False] * ni
    rng.shuffle(kinds)                                                    # allocation order mixes common and instance points
    names, kc, ki = [], 0, 0
    for c in kinds:
        names.append("G%d" % kc if c else "P%d" % ki)
        kc, ki = kc + c, ki + (not c)
    common = dict(zip(names, kinds))
    b = _Builder(b"random %d" % seed)
    b.points = list(zip(names, kinds))
    pool = [b.sec("x%d" % i) for i in range(int(rng.integers(1, 9)))]
    skew = [names[i] for i in rng.permutation(len(names))]                # the first names of this order are drawn most often
    draw = lambda seq: seq[int(len(seq) * rng.random() ** 3)]
    on_rhs, lhs_seen = set(), []
    for k in range(ncons):
        free = [p for p in names if p not in on_rhs]
        again = [p for p in lhs_seen if p in free]
        cand_i, cand_c = [p for p in free if not common[p]], [p for p in free if common[p]]
        u = rng.random()
        if again and u < 0.25:
            lhs = again[int(rng.integers(0, len(again)))]                # one point as left-hand side of two constraints
        elif cand_c and (u > 0.9 or not cand_i):
            lhs = cand_c[int(rng.integers(0, len(cand_c)))]              # a common left-hand side
        elif cand_i:
            lhs = cand_i[int(rng.integers(0, len(cand_i)))]
        else:
            break
        rhs_pool = [p for p in skew if p != lhs]
        pts = [draw(rhs_pool) for _ in range(int(rng.integers(1, 13)))]
        secs = [draw(pool) for _ in pts]
        if common[lhs] or lhs in lhs_seen:
            secs[int(rng.integers(0, len(secs)))] = b.sec("r%d" % k)     # the secret the reconciliation solves for
        b.con(lhs, pts, secs)
        on_rhs |= set(pts)
        lhs_seen.append(lhs)
    return b.shape()


_SHAPES = {}


def statement(key):
    """key: a family's name or a random statement's seed"""
    if key not in _SHAPES:
        _SHAPES[key] = FAMILIES[key]() if isinstance(key, str) else random_statement(key)
    return _SHAPES[key]


KEYS = list(FAMILIES) + list(SEEDS)


def sizes(key):
    """(n_small, n_big): both jobs below 1,024 terms (the generic classifier) / both at or above (the one-launch classifier), n_big even and
    beyond one wavefront of proofs.  static_uses_at_group_edge: N = 3 and N = 4, both above 1,024 terms."""
    if key == "static_uses_at_group_edge":
        return (3, 4)
    shape = statement(key)
    t = sum(len(lc) for _, lc in shape.cons)
    assert N_SMALL * (t + len(shape.cons)) < STMT_MIN_TERMS
    n = -(-STMT_MIN_TERMS // t)
    return (N_SMALL, max(66, n + (n & 1)))


# ---- values: a true statement ------------------------------------------------------------------------------------------------------------------------
def solve(shape, n, rng):
    """-> (secrets_int: name -> [n] ints, dlog: point name -> int (common) or [n] ints (instance)) of n proofs of a true statement"""
    r = lambda: int.from_bytes(rng.bytes(32), "little") % (L - 1) + 1
    common = dict(shape.points)
    lhs_names = {lhs for lhs, _ in shape.cons}
    dlog = {}
    for p, c in shape.points:
        if c:
            dlog[p] = r()
        elif p not in lhs_names:
            dlog[p] = [r() for _ in range(n)]
    sec = {s: [r() for _ in range(n)] for s in shape.secret_names}
    slots = collections.Counter(s for _, lc in shape.cons for s, _ in lc)
    val = lambda p, j: dlog[p] if common[p] else dlog[p][j]
    on_rhs = set()
    for lhs, lc in shape.cons:
        assert lhs not in on_rhs and all(p != lhs for _, p in lc), "a left-hand side never appears on an earlier or its own right-hand side"
        if lhs not in dlog:
            dlog[lhs] = [sum(sec[s][j] * val(p, j) for s, p in lc) % L for j in range(n)]
        else:
            q = next(i for i, (s, _) in enumerate(lc) if slots[s] == 1)       # a secret only this constraint uses, once
            s0, p0 = lc[q]
            for j in range(n):
                rest = sum(sec[s][j] * val(p, j) for i, (s, p) in enumerate(lc) if i != q)
                sec[s0][j] = (val(lhs, j) - rest) * pow(val(p0, j), -1, L) % L
        on_rhs |= {p for _, p in lc}
    return sec, dlog


class Case:
    """shape, n, secrets [n][m][32], inst [ni][n][32], common [ns][32]; ordinary = two of its own proofs (oracle_expectation's first batch of
    batch_verify_many); degenerate = {} and same_entropy = False: the attribute set of tests/degenerate_cases.py's Batch"""


def case(key, n):
    shape = statement(key)
    rng = np.random.default_rng([sum(str(key).encode()), n, 0xCA5E])
    sec, dlog = solve(shape, n, rng)
    b = Case()
    b.key, b.shape, b.n, b.same_entropy, b.degenerate = key, shape, n, False, {}
    b.secrets, b.inst, b.common = _materialise(shape, n, sec, dlog)
    b.ordinary = (b.secrets[:2].copy(), np.ascontiguousarray(b.inst[:, :2]))
    return b


# ---- what the plan must derive --------------------------------------------------------------------------------------------------------------------------
def _pair_terms(toff, tpt, ns, np_):
    from tests.test_host_stmt_pairs import _pairs
    cons = [[int(p) for p in tpt[toff[k]:toff[k + 1]]] for k in range(len(toff) - 1)]
    n, _, _, pair = _pairs(cons, ns, np_)
    return None if not n else [int(x) for x in pair]


class Census:
    """One job of a statement flow.  Point ids as in the plan: common points first, then instance points, each in allocation order.
    flow "prove": the terms are the right-hand sides (prover.rs:94-97); flow "verify": per constraint the right-hand side terms, then the
    left-hand side (verifier.rs:95-106), and -- pairs=True, what ZKP_OPT_JOINT_LADDER allows in calls of 1,024 terms or more -- pair[] says
    which terms ride on another term's doubling chain.  cnt[p] = terms of point p that do not ride, acnt[p] = those that do."""

    def __init__(self, shape, flow, pairs=True):
        assert flow in ("prove", "verify")
        self.shape, self.flow = shape, flow
        self.ns = sum(1 for _, c in shape.points if c)
        self.np = len(shape.points)
        kc, ki, self.id = 0, 0, {}
        for p, c in shape.points:
            self.id[p] = kc if c else self.ns + ki
            kc, ki = kc + c, ki + (not c)
        self.name = {i: p for p, i in self.id.items()}
        self.toff, self.tpt, self.tsec = [0], [], []
        for lhs, lc in shape.cons:
            for s, p in lc:
                self.tpt.append(self.id[p]), self.tsec.append(s)
            if flow == "verify":
                self.tpt.append(self.id[lhs]), self.tsec.append(None)     # (-c) on the left-hand side
            self.toff.append(len(self.tpt))
        self.T = len(self.tpt)
        self.pair = _pair_terms(self.toff, self.tpt, self.ns, self.np) if (flow == "verify" and pairs) else None
        self.cnt, self.acnt = [0] * self.np, [0] * self.np
        for k, p in enumerate(self.tpt):
            (self.acnt if self.rides(k) else self.cnt)[p] += 1

    def rides(self, k):
        return self.pair is not None and self.pair[k] != UNPAIRED and bool(self.pair[k] & ABSORBED)

    def per_proof(self):
        return range(self.ns, self.np)

    def comb_min(self, requested):
        """fused_flows.h: constant-time calls give single-use points a table (comb_min 1) only next to the table chains of a shared per-proof
        point; without one the ladder is cheaper -> 2.  Every other request is 2."""
        if requested == 1 and any(self.cnt[p] >= 2 for p in self.per_proof()):
            return 1
        return 2

    def is_rider(self, p, rider_ok):
        """stmt_pairs.h: a per-proof point ALL of whose terms ride, at least STMT_RIDER_MIN of them, in a job whose tables have 16 teeth"""
        return bool(rider_ok) and p >= self.ns and self.cnt[p] == 0 and self.acnt[p] >= STMT_RIDER_MIN

    def bounds(self, N, comb_min=2, riders=False):
        """cfg_from_terms: tables (one per common point, N per instance point) for points with comb_min or more uses (a common point's uses
        count N times) and for riders' points; ladders for single uses; pick_teeth: 16 teeth from two terms per table on, else 4"""
        comb_min = self.comb_min(comb_min)
        n_tab = n_lad = tab_terms = 0
        for p in range(self.np):
            mult = 1 if p < self.ns else N
            uses = self.cnt[p] * N if p < self.ns else self.cnt[p]
            if uses and uses >= comb_min:
                n_tab, tab_terms = n_tab + mult, tab_terms + uses * mult
            elif uses == 1:
                n_lad += mult
            if riders and self.is_rider(p, True):
                n_tab, tab_terms = n_tab + mult, tab_terms + self.acnt[p] * mult
        teeth = 16 if n_tab and tab_terms >= 2 * n_tab else 4
        return {"n_tab": n_tab, "n_lad": n_lad, "teeth": teeth, "comb_min": comb_min}

    def rider_ok(self, N, riders=True):
        """whether the classifier hands out riders' tables: pairs on, the caller asked for them, and the job's tables have 16 teeth"""
        return self.pair is not None and riders and self.bounds(N, 2, riders)["teeth"] == 16

    def classes(self, N, comb_min=2, group_min=NO_GROUPS, riders=False, registered=()):
        """-> {point name: "fixed" (a registered common point) | "group" | "comb" | "ladder" | "rider" (no term on a list, a table of
        multiples) | "none" (no term on a list, no table)}.  group_min counts only in constant-time jobs with 16-teeth tables."""
        k = self.bounds(N, comb_min, riders)
        if self.flow != "prove" or k["teeth"] != 16 or not k["n_tab"]:
            group_min = NO_GROUPS
        rider_ok = self.rider_ok(N, riders)
        out = {}
        for p in range(self.np):
            u = self.cnt[p] * N if p < self.ns else self.cnt[p]
            if p < self.ns and self.name[p] in registered:
                c = "fixed"
            elif self.cnt[p] == 0:
                c = "rider" if self.is_rider(p, rider_ok) else "none"
            else:
                c = "group" if u >= group_min else ("comb" if u >= k["comb_min"] else "ladder")
            out[self.name[p]] = c
        return out

    def line(self, N, **kw):
        k = self.bounds(N, **{a: b for a, b in kw.items() if a in ("comb_min", "riders")})
        used = [p for p in range(self.np) if self.cnt[p] + self.acnt[p]]
        if len(used) <= 24:
            pts = " ".join("%s:%d/%d" % (self.name[p], self.cnt[p], self.acnt[p]) for p in used)
        else:                                                             # (many points: how many common / per-proof points have each cnt/acnt)
            h = collections.Counter(("common" if p < self.ns else "per-proof", self.cnt[p], self.acnt[p]) for p in used)
            pts = " ".join("%dx%s:%d/%d" % (n, kind, c, a) for (kind, c, a), n in sorted(h.items()))
        return "%s N=%d T=%d pairs=%d n_tab=%d n_lad=%d teeth=%d comb_min=%d cnt/acnt %s" % (
            self.flow, N, self.T, 0 if self.pair is None else sum(self.rides(k_) for k_ in range(self.T)), k["n_tab"], k["n_lad"], k["teeth"], k["comb_min"], pts)


_CENSUS = {}


def census(shape, flow, pairs=True):
    key = (id(shape), flow, pairs)
    if key not in _CENSUS:
        _CENSUS[key] = (shape, Census(shape, flow, pairs))
    return _CENSUS[key][1]


def edges_of(shape):
    """the states of the issue's list that a statement reaches -> set of names"""
    v, p = census(shape, "verify"), census(shape, "prove")
    e = set()
    for q in v.per_proof():
        if v.cnt[q] == 0 and v.acnt[q] == STMT_RIDER_MIN:
            e.add("rider_at_min")
        if v.cnt[q] == 0 and v.acnt[q] == 1:
            e.add("rider_below_min")
        if v.acnt[q] >= 1 and v.cnt[q] == 1:
            e.add("partial_rider_leaves_one_use")
        if v.acnt[q] >= 1 and v.cnt[q] >= 2:
            e.add("partial_rider_leaves_two_uses")
    for u in (9, 10, 11):
        if any(p.cnt[q] == u for q in p.per_proof()):
            e.add("prover_uses_%d" % u)
    if len({p.cnt[q] for q in p.per_proof() if p.cnt[q] >= GROUP_MIN_USES}) >= 2:
        e.add("groups_of_different_sizes")
    if v.pair is not None and v.bounds(64, 2, True)["teeth"] == 4:
        e.add("four_teeth_with_pairs")
    uses = [v.cnt[q] + v.acnt[q] for q in range(v.np)]
    for k in range(len(shape.cons)):
        terms = range(v.toff[k], v.toff[k + 1])
        singles = [t for t in terms if v.tpt[t] >= v.ns and uses[v.tpt[t]] == 1]
        if v.pair is not None and len(singles) >= 3 and any(v.pair[t] == UNPAIRED for t in singles) and any(v.pair[t] != UNPAIRED for t in singles):
            e.add("odd_single_stays_unpaired")
    lhs = [l for l, _ in shape.cons]
    rhs = {q for _, lc in shape.cons for _, q in lc}
    if any(l in rhs for l in lhs):
        e.add("lhs_is_rhs_elsewhere")
    if any(lhs.count(l) >= 2 and dict(shape.points)[l] is False and v.acnt[v.id[l]] >= 1 for l in lhs):
        e.add("lhs_twice_and_rides")
    lens = [len(lc) for _, lc in shape.cons]
    if len(lens) >= 3 and min(lens) <= 2 and max(lens) >= 10:
        e.add("uneven_constraint_lengths")
    return e


RANDOM_EDGES = ("rider_at_min", "rider_below_min", "partial_rider_leaves_one_use", "partial_rider_leaves_two_uses", "prover_uses_9", "prover_uses_10",
                "prover_uses_11", "groups_of_different_sizes", "four_teeth_with_pairs", "odd_single_stays_unpaired", "lhs_is_rhs_elsewhere",
                "lhs_twice_and_rides", "uneven_constraint_lengths")


# ---- oracle expectations, one per (statement, n), shared by every test that needs them ----------------------------------------------------------------------
_EXPECT = {}


def _points_of(b, inst, j):
    inst_names = [p for p, c in b.shape.points if not c]
    common_names = [p for p, c in b.shape.points if c]
    return np.stack([b.common[common_names.index(p)] if c else inst[inst_names.index(p)][j] for p, c in b.shape.points])


def tamper_slot(shape):
    """the response to tamper with: the secret of a right-hand side term that rides where the statement has one, else of the first term"""
    v = census(shape, "verify")
    riding = [v.tsec[k] for k in range(v.T) if v.rides(k) and v.tsec[k] is not None]
    return shape.secret_names.index(riding[0] if riding else shape.cons[0][1][0][0])


def _tampered(b, E):
    """E with one response of proof n // 2 changed; the oracle says again what each verifier must answer.  Only that proof's verdicts can change:
    the others' inputs are the same bytes."""
    _, cst = b.shape.build()
    n, j = b.n, b.n // 2
    B = SH.OracleExpectation()
    B.__dict__.update(E.__dict__)
    B.resp, B.resp2, B.vc, B.vb = E.resp.copy(), E.resp2.copy(), E.vc.copy(), E.vb.copy()
    B.resp[j, tamper_slot(b.shape), 0] ^= 1
    B.resp2[n + j] = B.resp[j]
    B.bad = j
    pts = _points_of(b, b.inst, j)
    B.vc[j] = C.verify_compact(cst, E.tl, pts, B.chal[j], B.resp[j]) != 0
    B.vb[j] = C.verify_batchable(cst, E.tl, pts, B.coms[j], B.resp[j], B.w_each[j]) != 0
    B.rc_batch = int(C.batch_verify(cst, E.tl, n, b.inst, b.common, B.coms, B.resp, B.w) != 0)
    rc, osc, _ = C.batch_verify(cst, E.tl, n, b.inst, b.common, B.coms, B.resp, B.w, want_msm_inputs=True)
    B.coeffs = osc if (rc == 0 and n <= 512) else None
    B.rc_many = [E.rc_many[0], int(C.batch_verify(cst, E.tl, n, np.ascontiguousarray(B.inst2[:, n:]), b.common, B.coms2[n:], B.resp2[n:],
                                                  np.ascontiguousarray(B.w2[:, n:])) != 0)]
    # the _dev helper also verifies the batch of the proofs the oracle accepts one by one
    acc = B.vb == 0
    sub = lambda a, axis=0: np.ascontiguousarray(np.compress(acc, a, axis=axis))
    B.sub = (int(acc.sum()), sub(b.inst, 1), sub(B.coms), sub(B.resp), sub(B.w, 1))
    B.rc_sub = int(C.batch_verify(cst, E.tl, B.sub[0], B.sub[1], b.common, B.sub[2], B.sub[3], B.sub[4]) != 0)
    return B


def expectation(key, n):
    """-> (case, E: the oracle on its own honest proofs, E_bad: the same with one tampered response)"""
    if (key, n) not in _EXPECT:
        b = case(key, n)
        E = oracle_expectation(b.shape, n, b.secrets, b.inst, b.common, n + sum(str(key).encode()), b.ordinary, tl=b"random statements")
        E.sub, E.rc_sub = (n, b.inst, E.coms, E.resp, E.w), E.rc_batch
        _EXPECT[(key, n)] = (b, E, _tampered(b, E))
    return _EXPECT[(key, n)]


def honest(E):
    return not E.vc.any() and not E.vb.any() and E.rc_batch == 0 and E.rc_many == [0, 0]


def check_verifiers_vs_oracle(eng, b, E, routes=(("host", NEVER), ("fused", 0))):
    """the verifier flows of _check_flows_vs_oracle alone, on E's proofs (tampered ones: the prover has nothing to say about them)"""
    st, _ = b.shape.build()
    n, tl = b.n, E.tl
    out = {}
    for route, thr in routes:
        T.set_fused_min_batch(thr)
        try:
            ts2 = _fresh(tl, n)
            res = T.verify_compact_batch(eng, st, ts2, b.inst, b.common, E.chal, E.resp)
            ok, coeffs = T.batch_verify_coeffs(eng, st, _fresh(tl, n), b.inst, b.common, E.coms, E.resp, E.w)
            ts4 = _fresh(tl, n)
            each = T.verify_batchable_each(eng, st, ts4, b.inst, b.common, E.coms, E.resp, E.w_each)
            verd = T.batch_verify_many(eng, st, 2, _fresh(tl, 2 * n), E.inst2, b.common, E.coms2, E.resp2, E.w2)
            try:
                T.batch_verify(eng, st, _fresh(tl, n), b.inst, b.common, E.coms, E.resp, E.w)
                rc = 0
            except T.VerificationFailure:
                rc = 1
        finally:
            T.set_fused_min_batch(32)
        j = _first_diff(res, E.vc)
        assert j is None, "%s route: verify_compact says %d for proof %d, the oracle %d" % (route, res[j], j, E.vc[j])
        j = _first_diff(each, E.vb)
        assert j is None, "%s route: verify_batchable says %d for proof %d, the oracle %d" % (route, each[j], j, E.vb[j])
        assert rc == E.rc_batch and ok == (E.rc_batch == 0), "%s route: batch_verify %d / %r, the oracle %d" % (route, rc, ok, E.rc_batch)
        if E.coeffs is not None:
            j = _first_diff(coeffs, E.coeffs)
            assert j is None, "%s route: operand scalar %d of the batch verifier differs from the oracle's" % (route, j)
        assert verd.tolist() == E.rc_many, "%s route: batch_verify_many %r, the oracle %r" % (route, verd.tolist(), E.rc_many)
        out[route] = (ts2[E.vc == 0][:, :203], ts4[E.vb == 0][:, :203])
    first = routes[0][0]
    for route, _ in routes[1:]:
        for x, y in zip(out[first], out[route]):
            assert x.shape == y.shape and (x == y).all(), "%s and %s routes leave different transcripts" % (first, route)


def check_statement(eng, key, n, routes=(("host", NEVER), ("fused", 0))):
    """every flow on the honest proofs, the verifier flows on the tampered batch, all against the oracle"""
    b, E, E_bad = expectation(key, n)
    assert honest(E), "the oracle refuses its own honest proofs of %r at n = %d" % (key, n)
    try:
        _check_flows_vs_oracle(eng, b.shape, n, b.secrets, b.inst, b.common, E, routes=routes)
        check_verifiers_vs_oracle(eng, b, E_bad, routes=routes)
    except AssertionError as err:
        raise AssertionError("statement %r, n = %d: %s" % (key, n, err)) from err

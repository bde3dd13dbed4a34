"""tests/random_statements.py without a GPU: every family reaches the state it is named for (by the plain-Python census), 200 random
statements reach every class edge, the oracle accepts its own honest proofs of every statement the GPU tests run -- the condition they rest
on, checked where the reference alone decides it -- and the host backend agrees with the oracle on every family, so generator and
expectation are proven before a GPU sees them.  tests/test_gpu_random_statements.py runs the same statements on the device."""
import collections

import pytest

from oracle import cbind as C
from zkp_amd import toolbox as T
from tests import random_statements as R
from tests import statement_shapes as SH
from tests.random_statements import GROUP_MIN_USES, STMT_MIN_TERMS, UNPAIRED, census


@pytest.fixture(scope="module")
def host():
    C.build()
    return T.HostEngine()


def _ids(c, names):
    return [c.id[p] for p in names.split()]


def test_rider_at_min():
    sh = R.statement("rider_at_min")
    v, n = census(sh, "verify"), R.sizes("rider_at_min")[1]
    (p,) = _ids(v, "P")
    assert (v.cnt[p], v.acnt[p]) == (0, R.STMT_RIDER_MIN) and "rider_at_min" in R.edges_of(sh)
    assert v.rider_ok(n) and v.classes(n, riders=True)["P"] == "rider" and v.classes(n, riders=False)["P"] == "none"
    # the rider's table is counted like a comb table: one for G, one per proof for P
    assert v.bounds(n, 2, True)["n_tab"] == 1 + n and v.bounds(n, 2, False)["n_tab"] == 1 and v.bounds(n, 2, True)["n_lad"] == 2 * n


def test_rider_below_min():
    sh = R.statement("rider_below_min")
    v, n = census(sh, "verify"), R.sizes("rider_below_min")[1]
    (c1,) = _ids(v, "C1")
    assert (v.cnt[c1], v.acnt[c1]) == (0, 1) and v.rider_ok(n)          # 16 teeth, riders' tables on -- and still none for C1
    assert v.classes(n, riders=True)["C1"] == "none" and v.bounds(n, 2, True)["n_tab"] == 1


def test_partial_riders():
    for key, left, cls in (("partial_rider_leaves_one_use", 1, "ladder"), ("partial_rider_leaves_two_uses", 2, "comb")):
        sh = R.statement(key)
        v, n = census(sh, "verify"), R.sizes(key)[1]
        (p,) = _ids(v, "P")
        assert (v.cnt[p], v.acnt[p]) == (left, 1) and key in R.edges_of(sh)
        assert census(sh, "verify", pairs=False).cnt[p] == left + 1 >= 2     # what pair_terms counted: a point of several uses
        assert v.classes(n, riders=True)["P"] == cls
    # the one use left is a ladder the bounds must count: C1, P and nothing else per proof (D keeps a table)
    v = census(R.statement("partial_rider_leaves_one_use"), "verify")
    assert v.bounds(100, 2, True)["n_lad"] == 200 and v.bounds(100, 2, True)["n_tab"] == 100 + 2


def test_three_singles_one_constraint():
    sh = R.statement("three_singles_one_constraint")
    v = census(sh, "verify")
    assert "odd_single_stays_unpaired" in R.edges_of(sh)
    p, q, c = _ids(v, "P Q C")
    term = {v.tpt[k]: k for k in range(v.T)}
    assert v.pair[term[p]] == term[q] and v.rides(term[q]) and v.pair[term[c]] == UNPAIRED


def test_lhs_rides_elsewhere():
    sh = R.statement("lhs_rides_elsewhere")
    v = census(sh, "verify")
    assert {"lhs_is_rhs_elsewhere", "lhs_twice_and_rides"} <= R.edges_of(sh)
    a, a2 = _ids(v, "A A2")
    assert (v.cnt[a], v.acnt[a]) == (2, 1) and (v.cnt[a2], v.acnt[a2]) == (1, 1)
    assert [lhs for lhs, _ in sh.cons].count("A") == 2


def test_group_edges():
    sh = R.statement("group_edges_9_10_11")
    p, n = census(sh, "prove"), R.sizes("group_edges_9_10_11")[1]
    assert [p.cnt[i] for i in _ids(p, "P9 P10 P11")] == [9, 10, 11] == [GROUP_MIN_USES - 1, GROUP_MIN_USES, GROUP_MIN_USES + 1]
    cl = p.classes(n, comb_min=1, group_min=GROUP_MIN_USES)
    assert (cl["P9"], cl["P10"], cl["P11"]) == ("comb", "group", "group")
    assert set(p.classes(n, comb_min=1).values()) == {"comb", "none"}     # no grouped walk: comb tables for all (the left-hand sides are no terms of the prover)
    sh = R.statement("many_groups_mixed_sizes")
    p = census(sh, "prove")
    big = [p.cnt[q] for q in p.per_proof() if 10 <= p.cnt[q] <= 13]
    assert len(big) >= 5 and len(set(big)) >= 3 and sorted(big) == sorted(R.MANY_GROUPS_USES)
    assert list(p.classes(66, comb_min=2, group_min=GROUP_MIN_USES).values()).count("group") == 1 + len(big)      # (G: 13 x 66 uses)


def test_four_teeth_with_pairs():
    sh = R.statement("four_teeth_with_pairs")
    v, p, n = census(sh, "verify"), census(sh, "prove"), R.sizes("four_teeth_with_pairs")[1]
    assert v.pair is not None and sum(v.rides(k) for k in range(v.T)) == 4
    for riders in (False, True):
        assert v.bounds(n, 2, riders)["teeth"] == 4 and v.bounds(n, 2, riders)["n_tab"] == 0
    assert not v.rider_ok(n) and p.bounds(n, 1)["teeth"] == 4 and p.bounds(n, 1)["comb_min"] == 2
    assert set(p.classes(n, comb_min=1, group_min=GROUP_MIN_USES).values()) == {"ladder", "none"}


def test_uneven_constraint_lengths():
    sh = R.statement("uneven_constraint_lengths")
    assert [len(lc) for _, lc in sh.cons] == [2, 33, 1, 31, 7] and "uneven_constraint_lengths" in R.edges_of(sh)


def test_static_uses_at_group_edge():
    sh = R.statement("static_uses_at_group_edge")
    p, v = census(sh, "prove"), census(sh, "verify")
    assert R.sizes("static_uses_at_group_edge") == (3, 4) and 340 <= p.T <= 360
    assert all(p.cnt[g] == 3 and v.cnt[g] == 3 for g in range(p.ns)) and p.ns == 117
    for n, cls in ((3, "comb"), (4, "group")):
        assert n * p.T >= STMT_MIN_TERMS and n * v.T >= STMT_MIN_TERMS       # the one-launch classifier is on
        assert 3 * n == (9, 12)[n - 3]
        assert {p.classes(n, comb_min=2, group_min=GROUP_MIN_USES)["G%d" % g] for g in range(117)} == {cls}


def test_kitchen_sink():
    sh = R.statement("kitchen_sink")
    used_pts = {q for _, lc in sh.cons for _, q in lc} | {lhs for lhs, _ in sh.cons}
    unref = [(q, c) for q, c in sh.points if q not in used_pts]
    assert sorted(unref) == [("U0", True), ("W", False)]
    slots = collections.Counter(s for _, lc in sh.cons for s, _ in lc)
    assert slots["idle"] == 0 and "idle" in sh.secret_names
    assert len({q for _, lc in sh.cons for s, q in lc if s == "x"}) >= 3
    assert sh.cons[0][1].count(("y", "P")) == 2 and census(sh, "prove").cnt[census(sh, "prove").id["P"]] >= 3


def test_batch_sizes_sit_on_both_sides_of_the_one_launch_classifier():
    for key in R.KEYS:
        p, v = census(R.statement(key), "prove"), census(R.statement(key), "verify")
        small, big = R.sizes(key)
        assert big * p.T >= STMT_MIN_TERMS and big * v.T >= STMT_MIN_TERMS
        if key != "static_uses_at_group_edge":
            assert small * v.T < STMT_MIN_TERMS and small * p.T < STMT_MIN_TERMS and big % 2 == 0 and big > 64


def test_random_statements_reach_every_class_edge():
    """over 200 seeds every edge occurs; the twelve seeds the GPU tests use reach every one of them too"""
    seen = collections.Counter()
    shapes = [R.random_statement(s) for s in range(200)]
    for sh in shapes:
        seen.update(R.edges_of(sh))
    print(dict(seen))
    for e in R.RANDOM_EDGES:
        assert seen[e] >= 1, e
    gpu = set().union(*(R.edges_of(R.statement(s)) for s in R.SEEDS))
    assert set(R.RANDOM_EDGES) <= gpu
    # the stated ranges, and every use count from 1 to 12
    uses = set()
    for sh in shapes:
        ns = sum(1 for _, c in sh.points if c)
        assert 0 <= ns <= 6 and 1 <= len(sh.points) - ns <= 12 and 1 <= len(sh.cons) <= 8 and all(1 <= len(lc) <= 12 for _, lc in sh.cons)
        uses |= set(census(sh, "prove").cnt) | set(census(sh, "verify", pairs=False).cnt)
    assert set(range(1, 13)) <= uses
    assert R.random_statement(7).cons == R.random_statement(7).cons      # seeded


@pytest.mark.parametrize("key", R.KEYS, ids=[str(k) for k in R.KEYS])
def test_the_oracle_accepts_its_own_honest_proofs(key):
    for n in R.sizes(key):
        b, E, E_bad = R.expectation(key, n)
        assert not E.vc.any() and not E.vb.any() and E.rc_batch == 0 and E.rc_many == [0, 0], (key, n)
        # ... and refuses the tampered one, and only that one
        j = E_bad.bad
        assert E_bad.vc[j] == 1 and E_bad.vc.sum() == 1 and E_bad.vb[j] == 1 and E_bad.vb.sum() == 1 and E_bad.rc_batch == 1 and E_bad.rc_many == [0, 1]
        assert E_bad.rc_sub == 0 and E_bad.sub[0] == n - 1


def test_the_tampered_response_belongs_to_a_term_that_rides():
    for key in R.KEYS:
        sh = R.statement(key)
        v = census(sh, "verify")
        riding = {v.tsec[k] for k in range(v.T) if v.rides(k)} - {None}
        if riding:
            assert sh.secret_names[R.tamper_slot(sh)] in riding
    assert sum(1 for key in R.FAMILIES if census(R.statement(key), "verify").pair is not None) >= 10


@pytest.mark.parametrize("key", list(R.FAMILIES))
def test_families_on_the_host_backend_vs_oracle(host, key):
    R.check_statement(host, key, R.sizes(key)[0])


def test_the_checks_notice_one_wrong_byte_and_one_wrong_verdict(host):
    """not vacuous: the same helpers against an expectation with one byte of one commitment changed, and against the tampered batch with the
    tampered proof's verdict taken back"""
    b, E, E_bad = R.expectation("rider_at_min", R.N_SMALL)
    wrong = SH.OracleExpectation()
    wrong.__dict__.update(E.__dict__)
    wrong.coms = E.coms.copy()
    wrong.coms[3, 1, 7] ^= 0x10
    with pytest.raises(AssertionError, match="commitments of proof 3"):
        SH._check_flows_vs_oracle(host, b.shape, b.n, b.secrets, b.inst, b.common, wrong)
    wrong = SH.OracleExpectation()
    wrong.__dict__.update(E_bad.__dict__)
    wrong.vc = E.vc.copy()
    with pytest.raises(AssertionError, match="verify_compact says 1 for proof %d" % E_bad.bad):
        R.check_verifiers_vs_oracle(host, b, wrong)

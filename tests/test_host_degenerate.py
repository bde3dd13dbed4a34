"""Degenerate witnesses and coinciding points (tests/degenerate_cases.py) through every flow of the toolbox on the host backend, against
oracle/c (every proof, byte for byte; every verdict) and oracle/model.py (one proof per family).  No GPU needed; tests/test_gpu_degenerate.py
runs the same table on the device.  Expected verdicts come from the oracles alone; what is asserted about them here is only that the
table is not vacuous: at least one family is accepted whole and at least one is refused whole."""
import numpy as np
import pytest

from oracle import cbind as C
from oracle import model as M
from zkp_amd import toolbox as T
from tests import degenerate_cases as D
from tests import statement_shapes as SH

SIZES = (6, 70)
WHOLE = [(s, f, n) for s in D.STATEMENTS for f in D.families_of(s) for n in SIZES]
MIXED = [(s, n, b) for s in D.STATEMENTS for n in SIZES for b in range(len(D.mixed_plans(s, n)))]


@pytest.fixture(scope="module")
def host():
    C.build()
    return T.HostEngine()


def _names(b):
    return {j: "%s: %s" % fd for j, fd in b.degenerate.items()}


def check_model_sample(b, E, j):
    """oracle/model.py on proof j: the same proof from the raw witness bytes, and the same verify_compact verdict"""
    pts = D.points_of(b, j)
    mc, mr, mk = D.model_prove(b.shape, M.Transcript(E.tl), b.secrets[j], pts, E.entropy[j].tobytes())
    assert (mc == E.chal[j]).all() and (mr == E.resp[j]).all() and (mk == E.coms[j]).all(), "model and C oracle prove differently: proof %d (%s)" % (j, _names(b).get(j))
    assert D.model_verify_compact(b.shape, M.Transcript(E.tl), pts, E.chal[j], E.resp[j]) == E.vc[j], "model and C oracle disagree on proof %d (%s)" % (j, _names(b).get(j))


def test_the_table_has_a_recipe_or_a_reason_for_every_statement_and_family():
    """31 of the 248 (statement, family) pairs cannot be built; each carries its reason.  A new statement or family changes these counts."""
    assert len(D.STATEMENTS) == 8 and len(D.FAMILIES) == 31 and len(D.WITNESS_FAMILIES) == 19
    for (s, f), why in D.NOT_APPLICABLE.items():
        assert s in D.STATEMENTS and f in D.FAMILIES and why
    assert len(D.NOT_APPLICABLE) == 31 and len(WHOLE) == (8 * 31 - 31) * len(SIZES)
    assert list(D.WITNESS_ALL_SLOTS_TIED) == ["instance_lhs_twice"]
    for s in ("dleq_macro", "dleq_capi", "cmz10", "repeated_term", "lhs_is_rhs_elsewhere", "instance_lhs_twice"):
        assert all(D.applicable(s, f) for f in D.WITNESS_FAMILIES)
    # every pair that is not excused builds, every index named in the plan is degenerate, and each family is built by some statement
    for s in D.STATEMENTS:
        for f in D.families_of(s):
            assert len(D.whole_batch(s, f, 6, 1).degenerate) == 6
    assert all(any(D.applicable(s, f) for s in D.STATEMENTS) for f in D.FAMILIES)
    assert D.placement(6) == [0, 5] and D.placement(70) == [0, 31, 32, 63, 64, 69] and D.placement(4096) == [0, 31, 32, 63, 64, 255, 256, 4095]


def test_witnesses_reach_the_calls_unreduced():
    b = D.whole_batch("dleq_macro", "w:2^256-1", 6, 1)
    assert (b.secrets[:, 0] == 255).all()
    b = D.whole_batch("cmz10", "w:l", 70, 1)
    ints = [[int.from_bytes(x.tobytes(), "little") for x in row] for row in b.secrets]
    assert all(row.count(D.L) >= 1 for row in ints) and any(row.count(D.L) == 21 for row in ints)
    assert {i for row in ints for i, v in enumerate(row) if v == D.L} == set(range(21))          # every slot in turn at n = 70


@pytest.mark.parametrize("stname,fam,n", WHOLE, ids=["%s-%s-%d" % c for c in WHOLE])
def test_whole_family_batches_on_the_host_backend_vs_oracles(host, stname, fam, n):
    b = D.whole_batch(stname, fam, n, D.seed_of(stname, fam, n))
    E = SH.oracle_expectation(b.shape, n, b.secrets, b.inst, b.common, n, b.ordinary, same_entropy=b.same_entropy)
    SH._check_flows_vs_oracle(host, b.shape, n, b.secrets, b.inst, b.common, E, names=_names(b))
    check_model_sample(b, E, 0)
    check_model_sample(b, E, n - 1)
    if b.same_entropy:
        assert (E.chal == E.chal[0]).all() and (E.resp == E.resp[0]).all()


@pytest.mark.parametrize("stname,n,k", MIXED, ids=["%s-%d-batch%d" % c for c in MIXED])
def test_mixed_batches_on_the_host_backend_vs_oracles(host, stname, n, k):
    """degenerate proofs at the placement indices among ordinary ones: each changes its own verdict only"""
    plan = D.mixed_plans(stname, n)[k]
    b = D.build_batch(stname, n, plan, D.seed_of(stname, n, k))
    assert sorted(b.degenerate) == sorted(plan)
    E = SH.oracle_expectation(b.shape, n, b.secrets, b.inst, b.common, n + k, b.ordinary)
    ordinary = [j for j in range(n) if j not in plan]
    assert not E.vc[ordinary].any() and not E.vb[ordinary].any()            # the oracle accepts every ordinary proof of the batch
    SH._check_flows_vs_oracle(host, b.shape, n, b.secrets, b.inst, b.common, E, names=_names(b))
    check_model_sample(b, E, sorted(plan)[k % len(plan)])


@pytest.mark.parametrize("stname", ["dleq_capi", "cancelling_pair"])
def test_identity_points_are_refused_at_allocation_and_by_the_batch_calls(host, stname):
    """The object API refuses an identity point when it is allocated (mod.rs:191-193), before any arithmetic; the batch calls of the C ABI
    take the same bytes and must answer what the oracle answers."""
    with pytest.raises(T.VerificationFailure):
        T.Verifier(b"DLEQProof", T.Transcript(b"degenerate"), host).allocate_point(b"A", bytes(32))
    with pytest.raises(T.VerificationFailure):
        T.BatchVerifier(b"DLEQProof", 1, [T.Transcript(b"degenerate")], host).allocate_instance_point(b"A", [bytes(32)])
    fam = "zero_secrets" if stname == "dleq_capi" else "neg_cancel"
    b = D.whole_batch(stname, fam, 6, 9)
    assert (b.inst[[p for p, c in b.shape.points if not c].index("A")] == 0).all()
    E = SH.oracle_expectation(b.shape, 6, b.secrets, b.inst, b.common, 9, b.ordinary)
    assert E.vc.all() and E.vb.all() and E.rc_batch == 1 and E.rc_many == [0, 1]
    if fam == "neg_cancel":
        assert (E.coms[:, 0] == 0).all()                                    # the honest commitment of A = x P + x (-P) is the identity
    SH._check_flows_vs_oracle(host, b.shape, 6, b.secrets, b.inst, b.common, E, names=_names(b))


def test_the_oracle_accepts_some_families_whole_and_refuses_others():
    """Not vacuous: the C oracle alone (no code under test) on every whole-family batch of 6 proofs.  As read from mod.rs:186-221: an
    identity left-hand side is refused, everything else is accepted -- non-canonical witnesses included."""
    accepted, refused = set(), set()
    for stname, fam, n in WHOLE:
        if n != SIZES[0]:
            continue
        b = D.whole_batch(stname, fam, n, D.seed_of(stname, fam, n))
        E = SH.oracle_expectation(b.shape, n, b.secrets, b.inst, b.common, n, b.ordinary, same_entropy=b.same_entropy, many=False)
        if not E.vc.any() and not E.vb.any() and E.rc_batch == 0:
            accepted.add((stname, fam))
        if E.vc.all() and E.vb.all() and E.rc_batch == 1:
            refused.add((stname, fam))
    print("accepted whole:", len(accepted), "refused whole:", len(refused), sorted(refused))
    assert len(accepted) >= 1 and len(refused) >= 1
    assert ("cancelling_pair", "neg_cancel") in refused and ("dleq_macro", "zero_secrets") in refused
    assert all((s, "w:" + k) in accepted for s in ("cmz10", "dleq_macro") for k, _ in D.NON_CANONICAL if k not in ("l", "ql"))

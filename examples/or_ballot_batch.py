#!/usr/bin/env python3
"""N exponential-ElGamal ballots (C1, C2) = (r B, m B + r Y) with a HIDDEN vote m in {0, 1}: each carries a Cramer-Damgard-Schoenmakers
disjunction of two DLEQ statements, branch b claiming  C1 = r B  and  C2 - b B = r Y.  The constraint system of define_proof cannot
express an OR; the proof is written out of the batched toolbox calls, every transcript step the reference's TranscriptProtocol:

    per-ballot transcript   Transcript(DOMAIN); domain_sep; B, Y, C1, C2 appended    toolbox.domain_sep, append_point_vars(validate=True)
    the prover's nonces     k (real branch), c_sim, s_sim (simulated branch)         toolbox.witness_rng_scalars keyed with r: the reference's
                                                                                     synthetic nonces, bound to transcript and witness
    real commitments        (k B, k Y)                                               toolbox.basepoint_mul, point_mul
    simulated commitments   (s_sim B - c_sim C1, s_sim Y - c_sim (C2 - b' B))        toolbox.multiscalar_mul, 2 N sums of two terms
    the challenge           the four commitments appended, then c                    toolbox.append_blinding_commitments, challenge_scalars
    the real branch         c_real = c - c_sim,  s_real = k + c_real r               toolbox.scalar_muladd
    the proof               (c_0, c_1, s_0, s_1)
    the verifier            recomputes the four commitments s_b G - c_b P,           toolbox.multiscalar_mul, 4 N sums of two terms
                            re-derives c and checks c_0 + c_1 == c                   toolbox.challenge_scalars, scalar_muladd
    the tally               (sum C1, sum C2) over the accepted ballots, decrypted,   toolbox.point_sum, point_mul, point_sub, basepoint_dlog
                            its logarithm read off

Which branch is real is the voter's secret.  Putting the real and the simulated commitments, challenges and responses into branch order is
done here with numpy selects on the host: example-level code, NOT constant time in the vote.  A voter's client that must hide the vote from
its own machine's timing needs a masked select there.

With --host (or eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/or_ballot_batch.py [N] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"OR ballot example"
L = 2**252 + 27742317777372353535851937790883648493
ONE = np.frombuffer((1).to_bytes(32, "little"), np.uint8).copy()
MINUS_ONE = np.frombuffer((L - 1).to_bytes(32, "little"), np.uint8).copy()
COMMITMENT_LABELS = [b"T1_0", b"T2_0", b"T1_1", b"T2_1"]


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def statement_transcripts(eng, Y, C1, C2):
    """Every ballot's transcript up to its statement -> (blobs [N][208], rejected [N]): a ballot with an identity component is refused, as
    validate_and_append_point_var refuses it"""
    n = len(C1)
    B = np.frombuffer(BASEPOINT, np.uint8)
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    T.domain_sep(ts, b"or-ballot", eng=eng)
    rejected = np.zeros(n, np.uint8)
    for label, pts in ((b"B", np.tile(B, (n, 1))), (b"Y", np.tile(Y[0], (n, 1))), (b"C1", C1), (b"C2", C2)):
        rejected |= T.append_point_vars(eng, ts, label, pts, validate=True)
    return ts, rejected


def branch_points(eng, C2):
    """D_b = C2 - b B for b = 0, 1 -> [2][N][32]"""
    D1, bad = T.point_sub(eng, C2, np.frombuffer(BASEPOINT, np.uint8))
    assert not bad.any()
    return np.stack([C2, D1])


def commitments_from(eng, Y, C1, D, s, c, branch):
    """(s_j B - c_j C1_j,  s_j Y - c_j D[branch_j][j]) for every ballot: 2 N sums of two terms in one call -> ([N][32], [N][32])"""
    n = len(C1)
    j = np.arange(n, dtype=np.uint32)
    table = np.concatenate([np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32), Y, C1, D[0], D[1]])
    negc = T.scalar_muladd(eng, c, MINUS_ONE)
    scalars = np.ascontiguousarray(np.stack([s, negc, s, negc], axis=1)).reshape(4 * n, 32)
    pidx = np.stack([np.zeros(n, np.uint32), 2 + j, np.ones(n, np.uint32), 2 + n + np.asarray(branch, np.uint32) * n + j], axis=1).reshape(-1)
    out, bad = T.multiscalar_mul(eng, np.arange(0, 4 * n + 1, 2, dtype=np.uint32), scalars, pidx.astype(np.uint32), table, ZKP_CT)
    assert not bad.any()
    out = out.reshape(n, 2, 32)
    return np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1])


def challenge(eng, ts, coms):
    """append the four commitments as blinding commitments (branch order), then get_challenge"""
    for label, pts in zip(COMMITMENT_LABELS, coms):
        T.append_blinding_commitments(eng, ts, label, pts)
    return T.challenge_scalars(eng, ts, b"chal")


def prove(eng, Y, C1, C2, r, claimed, entropy=None):
    """The disjunction for every ballot, `claimed` [N] of 0 / 1 naming the branch proved with the witness r (an honest voter's is the vote)
    -> (c0, c1, s0, s1), each [N][32]"""
    n = len(C1)
    claimed = np.asarray(claimed, np.int64)
    D = branch_points(eng, C2)
    ts, rejected = statement_transcripts(eng, Y, C1, C2)
    assert not rejected.any()
    # the synthetic nonces of prover.rs:78-89: bound to the transcript so far, the witness and fresh entropy
    nonces = T.witness_rng_scalars(eng, ts, r.reshape(n, 1, 32), 3, entropy)
    k, c_sim, s_sim = (np.ascontiguousarray(nonces[:, i]) for i in range(3))
    real1 = T.basepoint_mul(eng, k)
    real2, bad = T.point_mul(eng, k, Y, ZKP_CT)
    assert not bad.any()
    sim1, sim2 = commitments_from(eng, Y, C1, D, s_sim, c_sim, 1 - claimed)
    # branch order (host selects on the secret branch: see the docstring)
    is0 = (claimed == 0)[:, None]
    coms = [np.where(is0, real1, sim1), np.where(is0, real2, sim2), np.where(is0, sim1, real1), np.where(is0, sim2, real2)]
    c = challenge(eng, ts, [np.ascontiguousarray(x) for x in coms])
    c_real = T.scalar_muladd(eng, c_sim, MINUS_ONE, c)                # c - c_sim
    s_real = T.scalar_muladd(eng, c_real, r, k)                       # k + c_real r
    return (np.where(is0, c_real, c_sim), np.where(is0, c_sim, c_real), np.where(is0, s_real, s_sim), np.where(is0, s_sim, s_real))


def verify(eng, Y, C1, C2, proof) -> np.ndarray:
    """-> accepted [N] of bool: the commitments recomputed from (c_b, s_b), c re-derived, c_0 + c_1 == c"""
    c0, c1, s0, s1 = (np.ascontiguousarray(x) for x in proof)
    n = len(C1)
    D = branch_points(eng, C2)
    ts, rejected = statement_transcripts(eng, Y, C1, C2)
    a1, a2 = commitments_from(eng, Y, C1, D, s0, c0, np.zeros(n, np.int64))
    b1, b2 = commitments_from(eng, Y, C1, D, s1, c1, np.ones(n, np.int64))
    c = challenge(eng, ts, [a1, a2, b1, b2])
    total = T.scalar_muladd(eng, c0, ONE, c1)
    return (total == c).all(axis=1) & (rejected == 0)


def encrypt(eng, Y, r, votes):
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    C2, bad2 = T.point_add(eng, rY, T.basepoint_mul(eng, scalar_rows(votes)))
    assert not bad.any() and not bad2.any()
    return C1, C2


def run(eng, n, key=None, votes=None, entropy=None, verbose=False):
    """N honest ballots and two bad ones, the board's checks and the tally.  eng = an Engine, or None for the host backend.  key (32 bytes)
    makes the secrets reproducible, votes [N] of 0 / 1 fixes the ballots, entropy [N + 2][32] the provers' entropy."""
    say = print if verbose else (lambda *a: None)
    if votes is None:
        votes = np.random.default_rng(n).integers(0, 2, size=n)
    votes = np.asarray(votes, np.int64)
    secrets = T.scalar_random(eng, n + 3, key)
    y, r, r_bad = secrets[:1], np.ascontiguousarray(secrets[1:n + 1]), np.ascontiguousarray(secrets[n + 1:])
    Y = T.basepoint_mul(eng, y)

    C1, C2 = encrypt(eng, Y, r, votes)
    proof = prove(eng, Y, C1, C2, r, votes, None if entropy is None else entropy[:n])
    say("%d ballots, each with a 128-byte disjunctive proof" % n)
    accepted = verify(eng, Y, C1, C2, proof)
    say("ballots verified: %d of %d" % (int(accepted.sum()), n))

    # two bad ballots: one encrypts m = 2 and claims branch 1; one is honest (m = 1) with c_0 and c_1 swapped
    X1, X2 = encrypt(eng, Y, r_bad, [2, 1])
    bad_proof = [np.array(x) for x in prove(eng, Y, X1, X2, r_bad, [1, 1], None if entropy is None else entropy[n:n + 2])]
    bad_proof[0][1], bad_proof[1][1] = bad_proof[1][1].copy(), bad_proof[0][1].copy()
    bad_ok = verify(eng, Y, X1, X2, bad_proof)
    say("m = 2 ballot: %s" % ("ACCEPTED" if bad_ok[0] else "rejected"))
    say("swapped c_0 ballot: %s" % ("ACCEPTED" if bad_ok[1] else "rejected"))

    # the tally over the accepted ballots: both components in one call, decrypted, its logarithm read off
    keep = np.flatnonzero(accepted)
    S, bad = T.point_sum(eng, np.array([0, len(keep), 2 * len(keep)], np.uint32), np.concatenate([C1[keep], C2[keep]]))
    assert not bad.any()
    Z, bad = T.point_mul(eng, y, S[:1], ZKP_CT)
    assert not bad.any()
    result, bad = T.point_sub(eng, S[1:], Z)
    assert not bad.any()
    count, status = T.basepoint_dlog(eng, result, max(1, int(n).bit_length()))
    tally = int(count[0]) if status[0] == 0 else -1
    say("tally: %d yes of %d (cast: %d)" % (tally, n, int(votes.sum())))
    return {"Y": Y, "C1": C1, "C2": C2, "proof": proof, "accepted": accepted, "bad_accepted": bad_ok, "count": tally, "cast": int(votes.sum())}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n = int(args[0]) if args else (64 if host else 4096)
    if host:
        run(None, n, verbose=True)
        return
    from zkp_amd.engine import Engine
    eng = Engine(0)
    try:
        run(eng, n, verbose=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

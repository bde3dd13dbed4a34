#!/usr/bin/env python3
"""N exponential-ElGamal ballots (C1, C2) = (r B, v B + r Y) with a HIDDEN vote v in {0 .. k-1}: each carries a 1-of-k OR-proof that it
encrypts one of the k values, by the batched flow of include/zkp_or_toolbox.h -- constant time in the vote, where examples/or_ballot_batch.py
(k = 2, written out of the single transcript calls) selects the branch order on the host.

    the statement        DLEQ over (B, C1; Y, D):  C1 = r B  and  D = r Y, with B and Y common
    branch b             D_b = C2 - b B                                                     toolbox.point_sub
    the proofs           challenges [N][k][32], responses [N][k][1][32]                     toolbox.or_prove, the voter's real = v
    the board's check    results [N]                                                        toolbox.or_verify
    two bad ballots      a vote of k proved on the false claim "branch 0", and an honest ballot with one response tampered
    the tally            (sum C1, sum C2) over the accepted ballots, decrypted,             toolbox.point_sum, point_mul, point_sub,
                         its logarithm read off: the sum of the votes                       basepoint_dlog

With --host (or eng = None in run()) everything runs on the host backend and needs no GPU; with an engine the proofs run on the GPU
whatever the default of toolbox.get_or_min_batch() is.

    python examples/vote_1_of_k_batch.py [N] [k] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = np.frombuffer(bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76"), np.uint8)
DOMAIN = b"1-of-k vote example"
L = T.L


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def statement() -> T.Statement:
    st = T.Statement(b"vote in range")
    r = st.add_secret(b"r")
    B, Y = st.add_point(b"B", True), st.add_point(b"Y", True)
    C1, D = st.add_point(b"C1", False), st.add_point(b"D", False)
    st.constrain(C1, [(r, B)])
    st.constrain(D, [(r, Y)])
    return st


def encrypt(eng, Y, r, votes):
    n = len(r)
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, np.tile(Y, (n, 1)), ZKP_CT)
    C2, bad2 = T.point_add(eng, rY, T.basepoint_mul(eng, scalar_rows(votes)))
    assert not bad.any() and not bad2.any()
    return C1, C2


def branch_points(eng, C1, C2, k) -> np.ndarray:
    """inst [k][2][N][32]: branch b is (C1, C2 - b B)"""
    n = len(C1)
    rows = [C2]
    for _ in range(1, k):
        D, bad = T.point_sub(eng, rows[-1], np.tile(BASEPOINT, (n, 1)))
        assert not bad.any()
        rows.append(D)
    return np.ascontiguousarray(np.stack([np.stack([C1, D]) for D in rows]))


def transcripts(n) -> np.ndarray:
    return np.stack([T.Transcript(DOMAIN).state] * n)


def run(eng, n, k=4, key=None, votes=None, entropy=None, verbose=False):
    """N honest ballots and two bad ones, the board's checks and the tally.  eng = an Engine, or None for the host backend.  key (32 bytes)
    makes the secrets reproducible, votes [N] of 0 .. k-1 fixes the ballots, entropy [N + 2][32] the provers' entropy."""
    say = print if verbose else (lambda *a: None)
    st = statement()
    if votes is None:
        votes = np.random.default_rng(n).integers(0, k, size=n)
    votes = np.asarray(votes, np.int64)
    secrets = T.scalar_random(eng, n + 3, key)
    y, r, r_bad = secrets[:1], np.ascontiguousarray(secrets[1:n + 1]), np.ascontiguousarray(secrets[n + 1:])
    Y = T.basepoint_mul(eng, y)[0]
    common = np.stack([BASEPOINT, Y])
    old = T.get_or_min_batch()
    if eng is not None:
        T.set_or_min_batch(0)
    try:
        C1, C2 = encrypt(eng, Y, r, votes)
        inst = branch_points(eng, C1, C2, k)
        chal, resp, status = T.or_prove(eng, st, transcripts(n), r.reshape(n, 1, 32), votes.astype(np.uint8), inst, common,
                                        None if entropy is None else entropy[:n])
        assert not status.any()
        say("%d ballots, each with a %d-byte 1-of-%d proof" % (n, 64 * k, k))
        accepted = T.or_verify(eng, st, transcripts(n), inst, common, chal, resp) == 0
        say("ballots verified: %d of %d" % (int(accepted.sum()), n))

        # two bad ballots: one encrypts v = k and claims branch 0; one is honest (v = 1 mod k) with a response tampered
        X1, X2 = encrypt(eng, Y, r_bad, [k, 1 % k])
        bad_inst = branch_points(eng, X1, X2, k)
        bchal, bresp, bstatus = T.or_prove(eng, st, transcripts(2), r_bad.reshape(2, 1, 32), np.array([0, 1 % k], np.uint8), bad_inst, common,
                                           None if entropy is None else entropy[n:n + 2])
        assert not bstatus.any()
        bresp[1, 0, 0] = scalar_rows([(int.from_bytes(bresp[1, 0, 0].tobytes(), "little") + 1) % L])[0]
        bad_ok = T.or_verify(eng, st, transcripts(2), bad_inst, common, bchal, bresp) == 0
    finally:
        T.set_or_min_batch(old)
    say("v = %d ballot: %s" % (k, "ACCEPTED" if bad_ok[0] else "rejected"))
    say("tampered ballot: %s" % ("ACCEPTED" if bad_ok[1] else "rejected"))

    # the tally over the accepted ballots: both components in one call, decrypted, its logarithm read off
    keep = np.flatnonzero(accepted)
    S, bad = T.point_sum(eng, np.array([0, len(keep), 2 * len(keep)], np.uint32), np.concatenate([C1[keep], C2[keep]]))
    assert not bad.any()
    Z, bad = T.point_mul(eng, y, S[:1], ZKP_CT)
    assert not bad.any()
    result, bad = T.point_sub(eng, S[1:], Z)
    assert not bad.any()
    count, st_ = T.basepoint_dlog(eng, result, max(1, int(n * max(1, k - 1)).bit_length()))
    tally = int(count[0]) if st_[0] == 0 else -1
    say("tally: %d (cast: %d)" % (tally, int(votes.sum())))
    return {"accepted": accepted, "bad_accepted": bad_ok, "count": tally, "cast": int(votes.sum()), "challenges": chal, "responses": resp}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n = int(args[0]) if args else (64 if host else 4096)
    k = int(args[1]) if len(args) > 1 else 4
    if host:
        run(None, n, k, verbose=True)
        return
    from zkp_amd.engine import Engine
    eng = Engine(0)
    try:
        run(eng, n, k, verbose=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The ballot box of examples/vote_1_of_k_batch.py with BATCHABLE 1-of-k proofs (include/zkp_or_batch_toolbox.h): every ballot carries its
commitments, so a tally server checks the whole box with ONE multiscalar sum instead of N k full recomputations, and only a box that
fails is searched for its bad ballots.

    the ballots          (C1, C2) = (r B, v B + r Y), v in {0 .. k-1} hidden                as vote_1_of_k_batch.py
    the proofs           commitments [N][k][2][32], challenges, responses                   toolbox.or_prove_batchable, real = v
    the box's check      one verdict                                                        toolbox.or_batch_verify
    two bad ballots      a vote of k proved on the false claim "branch 0", and an honest    the box then fails as a whole and
                         ballot with one response tampered, appended to the box             toolbox.or_batch_verify_locate names exactly those
    the tally            over the ballots that were not named                               toolbox.point_sum, point_mul, point_sub, basepoint_dlog

With --host everything runs on the host backend and needs no GPU; with an engine the proofs and the checks run on the GPU whatever the
defaults of toolbox.get_or_min_batch() and get_or_batch_min_batch() are.

    python examples/vote_1_of_k_tally_batch.py [N] [k] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import vote_1_of_k_batch as V
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT


def run(eng, n, k=4, key=None, votes=None, verbose=False):
    """N honest ballots, the box's batch check, the same box with two bad ballots appended, their localisation and the tally of the rest"""
    say = print if verbose else (lambda *a: None)
    st = V.statement()
    if votes is None:
        votes = np.random.default_rng(n).integers(0, k, size=n)
    votes = np.asarray(votes, np.int64)
    secrets = T.scalar_random(eng, n + 3, key)
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])                     # r: N honest ballots, then the two bad ones
    Y = T.basepoint_mul(eng, y)[0]
    common = np.stack([V.BASEPOINT, Y])
    all_votes = np.concatenate([votes, [k, 1 % k]])
    real = np.concatenate([votes, [0, 1 % k]]).astype(np.uint8)               # the v = k ballot claims branch 0
    old = T.get_or_min_batch(), T.get_or_batch_min_batch()
    if eng is not None:
        T.set_or_min_batch(0)
        T.set_or_batch_min_batch(0)
    try:
        C1, C2 = V.encrypt(eng, Y, r, all_votes)
        inst = V.branch_points(eng, C1, C2, k)
        coms, chal, resp, status = T.or_prove_batchable(eng, st, V.transcripts(n + 2), r.reshape(n + 2, 1, 32), real, inst, common)
        assert not status.any()
        resp[n + 1, 0, 0] = V.scalar_rows([(int.from_bytes(resp[n + 1, 0, 0].tobytes(), "little") + 1) % V.L])[0]
        say("%d ballots, each with a %d-byte batchable 1-of-%d proof" % (n, 128 * k, k))
        honest = np.ascontiguousarray(inst[:, :, :n])
        ok = T.or_batch_verify(eng, st, V.transcripts(n), honest, common, coms[:n], chal[:n], resp[:n])
        say("box of %d ballots: batch check %s" % (n, "passed" if ok else "FAILED"))
        ok_bad, results = T.or_batch_verify_locate(eng, st, V.transcripts(n + 2), inst, common, coms, chal, resp)
        say("box with 2 bad ballots: batch check %s" % ("PASSED" if ok_bad else "failed"))
        named = np.flatnonzero(results)
        say("located: ballots %s" % " and ".join(str(int(j)) for j in named))
    finally:
        T.set_or_min_batch(old[0])
        T.set_or_batch_min_batch(old[1])

    keep = np.flatnonzero(results == 0)
    S, bad = T.point_sum(eng, np.array([0, len(keep), 2 * len(keep)], np.uint32), np.concatenate([C1[keep], C2[keep]]))
    assert not bad.any()
    Z, bad = T.point_mul(eng, y, S[:1], ZKP_CT)
    assert not bad.any()
    result, bad = T.point_sub(eng, S[1:], Z)
    assert not bad.any()
    count, st_ = T.basepoint_dlog(eng, result, max(1, int(n * max(1, k - 1)).bit_length()))
    tally = int(count[0]) if st_[0] == 0 else -1
    say("tally: %d (cast: %d)" % (tally, int(votes.sum())))
    return {"ok": ok, "ok_bad": ok_bad, "named": named, "count": tally, "cast": int(votes.sum())}


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

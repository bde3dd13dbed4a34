#!/usr/bin/env python3
"""A verifiable yes / no tally over exponential ElGamal on ristretto255 for N ballots, every group operation a batched product call:

    election key      Y = y B                                    toolbox.basepoint_mul
    ballot j          (C1_j, C2_j) = (r_j B, r_j Y + v_j B)      toolbox.basepoint_mul, point_mul, point_add       v_j in {0, 1}
    its proof         the ballot encrypts the committed value M_j = v_j B:
                      C1_j = r_j B  and  C2_j - M_j = r_j Y       toolbox.point_sub makes the instance point, prove_batch the DLEQ
    the board         batch-verifies all N proofs                toolbox.batch_verify, verify_compact_batch
    the tally         (S1, S2) = (sum C1_j, sum C2_j)            toolbox.point_sum: two sums of N terms, one call
    its decryption    Z = y S1 with a proof that                 toolbox.point_mul, prove_batch with the SUM S1 as an instance point
                      Y = y B  and  Z = y S1
    the result        S2 - Z = (sum v_j) B                       toolbox.point_sub; the count is read off against k B, k = 0 .. N

The sums and differences are the calls of include/zkp_mi355x.h section 9; nothing builds a CSR job with scalars 1 and l - 1.  With --host (or
eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/elgamal_tally_batch.py [N] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"ElGamal tally example"


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def run(eng, n, key=None, votes=None, verbose=False):
    """N ballots, their proofs, the board's checks, the tally and its decryption proof.  eng = an Engine, or None for the host backend.  key
    (32 bytes) makes the secrets reproducible, votes [N] of 0 / 1 fixes the ballots.  Returns a dict of what was computed and the verdicts."""
    peng = eng if eng is not None else T.HostEngine()                # (the proof calls want an object in the engine's place)
    say = print if verbose else (lambda *a: None)
    enc = T.define_proof("ballot", b"ballot encrypts M", ["r"], ["C1", "D"], ["B", "Y"], [("C1", [("r", "B")]), ("D", [("r", "Y")])])
    dec = T.define_proof("decryption", b"tally decryption", ["y"], ["Y", "Z", "S1"], ["B"], [("Y", [("y", "B")]), ("Z", [("y", "S1")])])
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    if votes is None:
        votes = np.random.default_rng(n).integers(0, 2, size=n)
    votes = np.asarray(votes, np.int64)

    # the election key and the ballots
    secrets = T.scalar_random(eng, n + 1, key)
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)
    common = np.ascontiguousarray(np.concatenate([B, Y]))
    M = T.basepoint_mul(eng, scalar_rows(votes))                     # the committed values v_j B (the identity for a no)
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    C2, bad2 = T.point_add(eng, rY, M)
    assert not bad.any() and not bad2.any()

    # each ballot's proof: a DLEQ over (B, C1 ; Y, C2 - M)
    D, bad = T.point_sub(eng, C2, M)
    assert not bad.any()
    inst = np.ascontiguousarray(np.stack([C1, D]))
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    chal, resp, coms = T.prove_batch(peng, enc.statement, ts, r.reshape(n, 1, 32), inst, common)
    say("%d ballots with %d-byte compact proofs" % (n, 32 + 32 * enc.statement.m))

    # the bulletin board recomputes D from what is public and verifies: all at once, and ballot by ballot
    D_v, _ = T.point_sub(eng, C2, M)
    inst_v = np.ascontiguousarray(np.stack([C1, D_v]))
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    T.batch_verify(peng, enc.statement, ts, inst_v, common, coms, resp)          # raises on failure
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    accepted = int((T.verify_compact_batch(peng, enc.statement, ts, inst_v, common, chal, resp) == 0).sum())
    say("ballot proofs: batch verified, %d of %d accepted one by one" % (accepted, n))
    # a ballot that claims the other value is rejected: D moves by B
    flipped = T.basepoint_mul(eng, scalar_rows(1 - votes))
    D_x, _ = T.point_sub(eng, C2, flipped)
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    rejected = int((T.verify_compact_batch(peng, enc.statement, ts, np.ascontiguousarray(np.stack([C1, D_x])), common, chal, resp) != 0).sum())
    say("claiming the other value: %d of %d rejected" % (rejected, n))

    # the tally: both components in one call, two sums of N terms
    S, bad = T.point_sum(eng, np.array([0, n, 2 * n], np.uint32), np.concatenate([C1, C2]))
    assert not bad.any()
    S1, S2 = S[:1], S[1:]

    # decryption with its proof: the sum is an instance point
    Z, bad = T.point_mul(eng, y, S1, ZKP_CT)
    assert not bad.any()
    dinst = np.ascontiguousarray(np.stack([Y, Z, S1]))
    ts = np.stack([T.Transcript(DOMAIN).state])
    dchal, dresp, _ = T.prove_batch(peng, dec.statement, ts, y.reshape(1, 1, 32), dinst, B)
    S_v, _ = T.point_sum(eng, np.array([0, n, 2 * n], np.uint32), np.concatenate([C1, C2]))       # the verifier sums the board itself
    ts = np.stack([T.Transcript(DOMAIN).state])
    dec_ok = bool(T.verify_compact_batch(peng, dec.statement, ts, np.ascontiguousarray(np.stack([Y, Z, S_v[:1]])), B, dchal, dresp)[0] == 0)
    result, bad = T.point_sub(eng, S_v[1:], Z)
    assert not bad.any()
    table = T.basepoint_mul(eng, scalar_rows(range(n + 1)))          # k B for k = 0 .. N
    hits = np.flatnonzero((table == result[0]).all(axis=1))
    count = int(hits[0]) if len(hits) else -1
    say("decryption proof %s; tally: %d yes of %d (cast: %d)" % ("verified" if dec_ok else "REJECTED", count, n, int(votes.sum())))
    return {"Y": Y, "C1": C1, "C2": C2, "M": M, "D": D, "S1": S1, "S2": S2, "Z": Z, "result": result, "count": count, "cast": int(votes.sum()),
            "accepted": accepted, "rejected": rejected, "decryption_verified": dec_ok, "r": r, "y": y}


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

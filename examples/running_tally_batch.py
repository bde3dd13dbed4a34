#!/usr/bin/env python3
"""The running tally of K precincts of n exponential-ElGamal ballots on ristretto255: the ciphertext of the count after EVERY ballot, each one a
ciphertext that a decryption proof can be made over, every group operation a batched product call:

    ballots           (C1_kb, C2_kb) = (r_kb B, r_kb Y + v_kb B), v in {0, 1}   toolbox.basepoint_mul, point_mul, point_add
    running tallies   (R1_kb, R2_kb) = the sums of the ballots 0 .. b of k      two toolbox.point_cumsum calls, one segment per precinct
    decryption        v_k0 + .. + v_kb from R2_kb - y R1_kb                     toolbox.point_mul, point_sub, basepoint_dlog

The counts are compared with numpy.cumsum of the votes.  Without a scan the K n running ciphertexts take n calls of point_add, or a point_sum job
over all prefixes with K n (n + 1) / 2 terms.  Exit status 0 only if every running total comes out.  With --host everything runs on the host
backend and needs no GPU.

    python examples/running_tally_batch.py [K] [n] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def run(eng, precincts, n=64, key=None, verbose=False):
    """eng = an Engine, or None for the host backend.  Returns a dict of what was computed and the verdict."""
    say = print if verbose else (lambda *a: None)
    total = precincts * n
    votes = np.random.default_rng(total).integers(0, 2, size=(precincts, n)).astype(np.uint64)
    secrets = T.scalar_random(eng, 1 + total, key)
    y, r = np.ascontiguousarray(secrets[:1]), np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    vB = T.basepoint_mul(eng, scalar_rows(votes.reshape(-1)))
    C2, bad2 = T.point_add(eng, rY, vB)
    assert not bad.any() and not bad2.any()

    off = np.arange(precincts + 1, dtype=np.uint32) * n
    R1, s1 = T.point_cumsum(eng, off, C1)
    R2, s2 = T.point_cumsum(eng, off, C2)
    assert not s1.any() and not s2.any()
    say("%d running ciphertexts from two scans of %d terms (all prefixes as sums: %d terms each)" % (total, total, precincts * n * (n + 1) // 2))

    yR1, bad = T.point_mul(eng, y, R1, ZKP_CT)
    M, bad2 = T.point_sub(eng, R2, yR1)
    assert not bad.any() and not bad2.any()
    counts, status = T.basepoint_dlog(eng, M, max(4, int(n).bit_length()))
    want = np.cumsum(votes, axis=1).reshape(-1)
    right = int(((status == 0) & (counts == want)).sum())
    say("%d of %d running totals decrypted" % (right, total))
    return {"votes": votes, "R1": R1, "R2": R2, "counts": counts, "ok": right == total}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    precincts = int(args[0]) if args else (4 if host else 64)
    n = int(args[1]) if len(args) > 1 else (16 if host else 256)
    if host:
        res = run(None, precincts, n, verbose=True)
    else:
        from zkp_amd.engine import Engine
        eng = Engine(0)
        try:
            res = run(eng, precincts, n, verbose=True)
        finally:
            eng.close()
    sys.exit(0 if res["ok"] else 1)


if __name__ == "__main__":
    main()

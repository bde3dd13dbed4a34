#!/usr/bin/env python3
"""Weighted tallies of K contests over exponential ElGamal on ristretto255, M ballots each, every group operation a batched product call:

    election key      Y = y B                                            toolbox.basepoint_mul
    ballot (k, j)     (C1, C2) = (r B, r Y + v B), v in {0, 1}           toolbox.basepoint_mul, point_mul, point_add
    public weights    w_kj: the voting power of ballot j of contest k   (shares, stake, seats -- known to everybody)
    the tallies       (S1_k, S2_k) = (sum_j w_kj C1_kj, sum_j w_kj C2_kj)
                      2 K multiscalar sums of M terms with PUBLIC scalars and a point per term: toolbox.optional_multiscalar_mul, one call;
                      on an engine with long segments that is zkp_msm_optional_many, the bucket method on K segments side by side
    the decryption    S2_k - y S1_k = (sum_j w_kj v_kj) B                toolbox.point_mul, point_sub
    the amounts       sum_j w_kj v_kj, read off with                     toolbox.basepoint_dlog

The weights are public, so the sums may run in variable time; the votes and the randomness never enter a variable-time call.  With --host (or
eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/contest_tallies_batch.py [K] [M] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
WEIGHT_BITS = 10


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def run(eng, K, M, key=None, verbose=False):
    """K contests of M ballots.  eng = an Engine, or None for the host backend; key (32 bytes) makes the secrets reproducible.  Returns a dict of
    what was computed: the amounts read off the tallies and the amounts counted from the votes in the clear."""
    say = print if verbose else (lambda *a: None)
    n = K * M
    rng = np.random.default_rng(1000 * K + M)
    votes = rng.integers(0, 2, size=n)
    weights = rng.integers(1, 1 << WEIGHT_BITS, size=n)

    secrets = T.scalar_random(eng, n + 1, key)
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    C2, bad2 = T.point_add(eng, rY, T.basepoint_mul(eng, scalar_rows(votes)))
    assert not bad.any() and not bad2.any()

    # 2 K weighted sums of M terms: segments 0 .. K - 1 over the C1 rows, K .. 2 K - 1 over the C2 rows; a point per term (pidx = None)
    off = (np.arange(2 * K + 1, dtype=np.uint64) * M).astype(np.uint32)
    w = scalar_rows(weights)
    S, bad = T.optional_multiscalar_mul(eng, off, np.concatenate([w, w]), np.concatenate([C1, C2]))
    assert not bad.any()
    S1, S2 = S[:K], S[K:]

    Z, bad = T.point_mul(eng, y, S1, ZKP_CT)
    assert not bad.any()
    result, bad = T.point_sub(eng, S2, Z)
    assert not bad.any()
    bits = WEIGHT_BITS + max(1, int(M).bit_length())
    amounts, st = T.basepoint_dlog(eng, result, bits)
    assert not st.any()
    counted = (weights * votes).reshape(K, M).sum(axis=1)
    ok = [int(a) for a in amounts] == [int(c) for c in counted]
    say("%d contests of %d ballots: weighted amounts %s%s" % (K, M, [int(a) for a in amounts[:8]], " ..." if K > 8 else ""))
    say("the tallies and the count in the clear %s" % ("agree" if ok else "DISAGREE"))
    return {"Y": Y, "C1": C1, "C2": C2, "S1": S1, "S2": S2, "amounts": amounts, "counted": counted, "agree": ok}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    K = int(args[0]) if args else (3 if host else 16)
    M = int(args[1]) if len(args) > 1 else (40 if host else 4096)
    if host:
        ok = run(None, K, M, verbose=True)["agree"]
    else:
        from zkp_amd.engine import Engine
        eng = Engine(0)
        try:
            ok = run(eng, K, M, verbose=True)["agree"]
        finally:
            eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

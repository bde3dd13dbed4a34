#!/usr/bin/env python3
"""K vector Pedersen commitments over one set of generators on ristretto255, and the verifier's aggregate check, every group operation a batched
product call:

    generators        G_0 .. G_{n-1}, H = hash_from_bytes::<Sha512>(labels)      toolbox.hash_from_bytes_sha512
    commitments       C_k = sum_i m_ki G_i + r_k H,  k < K                        toolbox.multiscalar_sum, ZKP_CT: K segments of n + 1 terms that
                                                                                  share the n + 1 points through pidx
    the check         sum_k w_k C_k == sum_i (sum_k w_k m_ki) G_i + (sum_k w_k r_k) H   for random weights w_k
      left side       one variable-time segment of K terms, a point per term      toolbox.multiscalar_sum, pidx = None
      right side      one segment of n + 1 terms                                  toolbox.multiscalar_sum; its scalars from toolbox.scalar_muladd

The sums are the call of include/zkp_mi355x.h section 11: the segments are long, so the term axis is folded in levels instead of being added by one
lane per sum.  With --host (or eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/pedersen_vector_batch.py K [n] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT, ZKP_VARTIME

DOMAIN = b"Pedersen vector example"


def run(eng, K, n, key=None, verbose=False):
    """K commitments to vectors of n scalars and the aggregate check.  eng = an Engine, or None for the host backend; key (32 bytes) makes the
    secrets reproducible.  Returns a dict of what was computed and the verdicts."""
    say = print if verbose else (lambda *a: None)
    gens = T.hash_from_bytes_sha512(eng, [DOMAIN + b" G %d" % i for i in range(n)] + [DOMAIN + b" H"])          # G_0 .. G_{n-1}, H
    secrets = T.scalar_random(eng, K * (n + 1), key)                  # row k (n + 1) + i = m_ki, the last of each block r_k
    off = (np.arange(K + 1, dtype=np.uint64) * (n + 1)).astype(np.uint32)
    pidx = np.tile(np.arange(n + 1, dtype=np.uint32), K)
    C, bad = T.multiscalar_sum(eng, off, secrets, gens, pidx, flags=ZKP_CT)
    assert not bad.any()
    say("%d commitments to %d scalars each over %d shared generators" % (K, n, n + 1))

    # the verifier: random weights, both sides of the aggregate equation
    w = T.scalar_random(eng, K, key, nonce=1)
    lhs, bad = T.multiscalar_sum(eng, np.array([0, K], np.uint32), w, C, None, flags=ZKP_VARTIME)
    assert not bad.any()
    acc = None                                                        # acc_i = sum_k w_k m_ki (i < n), acc_n = sum_k w_k r_k
    for k in range(K):
        acc = T.scalar_muladd(eng, w[k], secrets[k * (n + 1):(k + 1) * (n + 1)], acc)
    rhs, bad = T.multiscalar_sum(eng, np.array([0, n + 1], np.uint32), acc, gens, None, flags=ZKP_VARTIME)
    assert not bad.any()
    agree = bool((lhs == rhs).all())
    # an opening that is off by one in one place does not pass
    wrong = acc.copy()
    wrong[0, 0] ^= 1
    rhs_x, _ = T.multiscalar_sum(eng, np.array([0, n + 1], np.uint32), wrong, gens, None, flags=ZKP_VARTIME)
    rejected = not bool((lhs == rhs_x).all())
    say("aggregate check: both sides %s; a wrong opening is %s" % ("agree" if agree else "DISAGREE", "rejected" if rejected else "ACCEPTED"))
    return {"generators": gens, "C": C, "w": w, "lhs": lhs, "rhs": rhs, "agree": agree, "rejected": rejected}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    K = int(args[0]) if args else 64
    n = int(args[1]) if len(args) > 1 else 1024
    if host:
        r = run(None, K, n, verbose=True)
    else:
        from zkp_amd.engine import Engine
        eng = Engine(0)
        try:
            r = run(eng, K, n, verbose=True)
        finally:
            eng.close()
    sys.exit(0 if r["agree"] and r["rejected"] else 1)


if __name__ == "__main__":
    main()

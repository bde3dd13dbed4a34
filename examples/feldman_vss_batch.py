#!/usr/bin/env python3
"""Feldman verifiable secret sharing of N secrets t-of-n on ristretto255, every scalar and group operation a batched product call:

    commitments       C_ki = c_ki B for the coefficients of secret k        toolbox.basepoint_mul
    powers            j^i for trustee j = 1 .. n, i = 0 .. t - 1            toolbox.scalar_powers: one exclusive product scan over t references to row j
    shares            s_kj = sum_i c_ki j^i                                 toolbox.scalar_dot over the table of powers, c gathered by index
    the check         s_kj B == sum_i j^i C_ki for every trustee            toolbox.basepoint_mul against toolbox.multiscalar_sum over the shared C_ki

The table of powers is also built the way examples/threshold_elgamal_batch.py builds it -- toolbox.scalar_product over "i references to row j",
t (t - 1) / 2 terms per trustee -- and must be the same bytes.  One share is then tampered with and must fail its check.  Exit status 0 only if
every honest share verifies, the tampered one does not and the two tables agree.  With --host everything runs on the host backend and needs no GPU.

    python examples/feldman_vss_batch.py [N] [t] [n] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_VARTIME


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def powers_by_products(eng, x, t):
    """the quadratic route: segment (j, i) references row j i times"""
    n = len(x)
    lens = np.tile(np.arange(t, dtype=np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    return T.scalar_product(eng, off, x, np.repeat(np.repeat(np.arange(n, dtype=np.uint32), t), lens)).reshape(n, t, 32)


def run(eng, n_secrets, t=3, n=5, key=None, verbose=False):
    """eng = an Engine, or None for the host backend.  Returns a dict of what was computed and the verdicts."""
    assert 2 <= t <= n
    say = print if verbose else (lambda *a: None)
    coeff = T.scalar_random(eng, n_secrets * t, key)                                        # row k t + i = c_ki; c_k0 is secret k
    C = T.basepoint_mul(eng, coeff)
    x = scalar_rows(range(1, n + 1))                                                        # trustee j evaluates at x_j = j

    powers = T.scalar_powers(eng, x, t)                                                     # [n][t][32]
    tables_agree = bool((powers == powers_by_products(eng, x, t)).all())
    say("a table of %d powers from one scan of %d terms; the product route takes %d terms and gives %s bytes"
        % (n * t, n * t, n * t * (t - 1) // 2, "the same" if tables_agree else "OTHER"))

    # share (k, j) is output k n + j; term i of it is c_ki * j^i
    k_of = np.repeat(np.arange(n_secrets, dtype=np.uint32), n * t)
    j_of = np.tile(np.repeat(np.arange(n, dtype=np.uint32), t), n_secrets)
    i_of = np.tile(np.arange(t, dtype=np.uint32), n_secrets * n)
    off = np.arange(n_secrets * n + 1, dtype=np.uint32) * t
    flat = np.ascontiguousarray(powers.reshape(n * t, 32))
    shares = T.scalar_dot(eng, off, coeff, flat, aidx=k_of * t + i_of, bidx=j_of * t + i_of)

    def verified(s):
        lhs = T.basepoint_mul(eng, s)
        rhs, bad = T.multiscalar_sum(eng, off, np.ascontiguousarray(flat[j_of * t + i_of]), C, k_of * t + i_of, ZKP_VARTIME)
        assert not bad.any()
        return (lhs == rhs).all(axis=1)

    ok = verified(shares)
    say("%d of %d shares verified" % (int(ok.sum()), len(ok)))
    forged = shares.copy()
    victim = len(forged) // 2
    forged[victim, 0] ^= 1
    ok_forged = verified(forged)
    forged_caught = bool(not ok_forged[victim] and ok_forged.sum() == len(ok_forged) - 1)
    say("a tampered share %s" % ("fails its check" if forged_caught else "PASSES"))
    return {"powers": powers, "shares": shares, "commitments": C, "coeff": coeff, "ok": ok, "tables_agree": tables_agree, "forged_caught": forged_caught}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n_secrets = int(args[0]) if args else (8 if host else 256)
    t = int(args[1]) if len(args) > 1 else 3
    n = int(args[2]) if len(args) > 2 else 5
    if host:
        r = run(None, n_secrets, t, n, verbose=True)
    else:
        from zkp_amd.engine import Engine
        eng = Engine(0)
        try:
            r = run(eng, n_secrets, t, n, verbose=True)
        finally:
            eng.close()
    sys.exit(0 if r["ok"].all() and r["tables_agree"] and r["forged_caught"] else 1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""t-of-n threshold decryption of N exponential-ElGamal amounts on ristretto255, every scalar and group operation a batched product call:

    powers            j^i for trustee j = 1 .. n, i = 0 .. t - 1        toolbox.scalar_product: segment (j, i) references row j i times
    Shamir shares     s_j = sum_i c_i j^i,  c_0 = y                     toolbox.scalar_dot over the table of powers, c gathered by index
    ciphertexts       (C1_k, C2_k) = (r_k B, r_k Y + m_k B)             toolbox.basepoint_mul, point_mul, point_add
    partial           D_jk = s_j C1_k for the trustees of a subset      toolbox.point_mul
    Lagrange          lambda_j = prod_{m != j} m / (m - j)              toolbox.scalar_product for numerators and denominators, the differences
                                                                        m - j = (l - 1) j + m by toolbox.scalar_muladd, then toolbox.scalar_invert
    the check         sum_j lambda_j s_j == y                           toolbox.scalar_dot
    combination       Z_k = sum_j lambda_j D_jk                         toolbox.multiscalar_sum
    the amounts       m_k B = C2_k - Z_k, then m_k                      toolbox.point_sub, toolbox.basepoint_dlog

A subset of t - 1 trustees must fail: its Lagrange combination of shares is not y and its amounts do not come out.  Exit status 0 only if the full
subset decrypts every amount and the short one does not.  With --host everything runs on the host backend and needs no GPU.

    python examples/threshold_elgamal_batch.py [N] [t] [n] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT, ZKP_VARTIME

L = 2 ** 252 + 27742317777372353535851937790883648493
BITS = 16


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def lagrange_at_zero(eng, x, subset):
    """lambda_j = prod_{m != j} x_m / (x_m - x_j) over the trustees of `subset` (indices into x [n][32]) -> [len(subset)][32]"""
    k = len(subset)
    others = np.array([[m for m in subset if m != j] for j in subset], np.uint32)          # [k][k - 1]
    off = np.arange(k + 1, dtype=np.uint32) * (k - 1)
    num = T.scalar_product(eng, off, x, others.reshape(-1))
    xj = np.ascontiguousarray(x[np.repeat(np.array(subset), k - 1)])
    xm = np.ascontiguousarray(x[others.reshape(-1)])
    diff = T.scalar_muladd(eng, xj, scalar_rows([L - 1])[0], xm)                            # x_m - x_j, one row per pair
    den = T.scalar_product(eng, off, diff)
    return T.scalar_muladd(eng, num, T.scalar_invert(eng, den))


def decrypt(eng, subset, shares, x, C1, C2, n_amounts):
    """the subset's partial decryptions combined: (lambda, sum lambda_j s_j, amounts, dlog status)"""
    k = len(subset)
    lam = lagrange_at_zero(eng, x, subset)
    s = np.ascontiguousarray(shares[np.array(subset)])
    secret = T.scalar_dot(eng, np.array([0, k], np.uint32), lam, s)
    D = []
    for j in range(k):
        d, bad = T.point_mul(eng, s[j], C1, ZKP_CT)
        assert not bad.any()
        D.append(d)
    D = np.concatenate(D)                                                                   # row j N + k' = D_jk'
    off = np.arange(n_amounts + 1, dtype=np.uint32) * k
    pidx = (np.arange(k, dtype=np.uint32)[None, :] * n_amounts + np.arange(n_amounts, dtype=np.uint32)[:, None]).reshape(-1)
    Z, bad = T.multiscalar_sum(eng, off, np.tile(lam, (n_amounts, 1)), D, pidx, ZKP_VARTIME)
    assert not bad.any()
    M, bad = T.point_sub(eng, C2, Z)
    assert not bad.any()
    amounts, status = T.basepoint_dlog(eng, M, BITS)
    return lam, secret, amounts, status


def run(eng, n_amounts, t=3, n=5, key=None, verbose=False):
    """eng = an Engine, or None for the host backend.  Returns a dict of what was computed and the verdicts."""
    assert 3 <= t <= n, "the short subset has t - 1 >= 2 trustees"
    say = print if verbose else (lambda *a: None)
    amounts = np.random.default_rng(n_amounts).integers(0, 1 << BITS, size=n_amounts).astype(np.uint64)
    secrets = T.scalar_random(eng, t + n_amounts, key)
    coeff, r = np.ascontiguousarray(secrets[:t]), np.ascontiguousarray(secrets[t:])         # c_0 = y, c_1 .. c_{t-1}
    y = coeff[:1]
    x = scalar_rows(range(1, n + 1))                                                        # trustee j evaluates at x_j = j

    # 1. the table of powers x_j^i (row j t + i) and the shares
    lens = np.tile(np.arange(t, dtype=np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    powers = T.scalar_product(eng, off, x, np.repeat(np.repeat(np.arange(n, dtype=np.uint32), t), lens))
    shares = T.scalar_dot(eng, np.arange(n + 1, dtype=np.uint32) * t, coeff, powers, aidx=np.tile(np.arange(t, dtype=np.uint32), n))
    say("%d shares of a degree-%d polynomial from a table of %d powers" % (n, t - 1, n * t))

    # the ciphertexts
    Y = T.basepoint_mul(eng, y)
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    mB = T.basepoint_mul(eng, scalar_rows(amounts))
    C2, bad2 = T.point_add(eng, rY, mB)
    assert not bad.any() and not bad2.any()

    # 2. - 7. a subset of t trustees decrypts
    subset = list(range(n - t, n))
    lam, secret, got, status = decrypt(eng, subset, shares, x, C1, C2, n_amounts)
    shares_ok = bool((secret == y).all())
    decrypted = bool((status == 0).all() and (got == amounts).all())
    say("trustees %s: sum lambda_j s_j %s y; %d of %d amounts decrypted" % ([j + 1 for j in subset], "==" if shares_ok else "!=", int(((status == 0) & (got == amounts)).sum()), n_amounts))

    # a subset of t - 1 trustees does not
    short = subset[1:]
    _, secret_x, got_x, status_x = decrypt(eng, short, shares, x, C1, C2, n_amounts)
    short_secret_differs = not bool((secret_x == y).all())
    short_right = int(((status_x == 0) & (got_x == amounts)).sum())
    say("trustees %s: sum lambda_j s_j %s y; %d of %d amounts decrypted" % ([j + 1 for j in short], "!=" if short_secret_differs else "==", short_right, n_amounts))
    return {"powers": powers, "shares": shares, "lambda": lam, "y": y, "amounts": amounts, "got": got, "shares_ok": shares_ok, "decrypted": decrypted,
            "short_fails": short_secret_differs and short_right == 0, "coeff": coeff, "x": x}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n_amounts = int(args[0]) if args else (16 if host else 256)
    t = int(args[1]) if len(args) > 1 else 3
    n = int(args[2]) if len(args) > 2 else 5
    if host:
        r = run(None, n_amounts, t, n, verbose=True)
    else:
        from zkp_amd.engine import Engine
        eng = Engine(0)
        try:
            r = run(eng, n_amounts, t, n, verbose=True)
        finally:
            eng.close()
    sys.exit(0 if r["shares_ok"] and r["decrypted"] and r["short_fails"] else 1)


if __name__ == "__main__":
    main()

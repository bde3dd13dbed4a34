#!/usr/bin/env python3
"""Net balances of N accounts from encrypted SIGNED transfers, under exponential ElGamal over a generator H of the deployment's own on
ristretto255, every group operation a batched call:

    the generator     H = hash_from_bytes::<Sha512>(label)                 toolbox.hash_from_bytes_sha512
    the key           Y = y B                                            toolbox.basepoint_mul
    transfer t        (C1_t, C2_t) = (r_t B, r_t Y + a_t H)              toolbox.basepoint_mul, point_mul, point_add    a_t of either sign
    account j         (C1_j, C2_j) = the sums over its transfers         toolbox.point_sum
    its decryption    Z_j = y C1_j with a proof that                     toolbox.point_mul, prove_batch: a DLEQ over (B, Y ; C1_j, Z_j)
                      Y = y B  and  Z_j = y C1_j
    the auditor       batch-verifies all N decryption proofs             toolbox.batch_verify, verify_compact_batch
    the net amounts   C2_j - Z_j = s_j H,  s_j = log_H, signed           toolbox.point_sub, toolbox.point_dlog(eng, H, ..., signed=True)

The last step is zkp_dlog_point of include/zkp_mi355x.h section 10: the amount sits on H, not on B (B carries the randomness), and a net balance
is signed, in [-2^(bits - 1), 2^(bits - 1)).  The signed search starts at 0 and works outward, so balances near zero -- most of them, in a ledger
of transfers that cancel -- are found by the first launches.  An account whose balance is outside the range comes back with status 2.
With --host (or eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/net_balances_batch.py [N] [bits] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"net balances example"
H_LABEL = b"net balances example: value generator"
L = 2**252 + 27742317777372353535851937790883648493
TRANSFERS = 3                                                            # per account


def scalar_rows(values) -> np.ndarray:
    """integers of either sign as scalars mod l"""
    return np.frombuffer(b"".join((int(v) % L).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def run(eng, n, bits=16, key=None, transfers=None, verbose=False):
    """N accounts of TRANSFERS encrypted transfers each, the decryption proofs of the summed ciphertexts, the auditor's checks and the recovered
    net balances.  eng = an Engine, or None for the host backend.  key (32 bytes) makes the secrets reproducible, transfers [N][TRANSFERS]
    fixes the plaintexts (an account whose sum is outside [-2^(bits - 1), 2^(bits - 1)) is reported as out of range; by default the last one is).
    Returns a dict of what was computed and the verdicts."""
    peng = eng if eng is not None else T.HostEngine()                # (the proof calls want an object in the engine's place)
    say = print if verbose else (lambda *a: None)
    dec = T.define_proof("decryption", b"balance decryption", ["y"], ["Y", "Z", "C1"], ["B"], [("Y", [("y", "B")]), ("Z", [("y", "C1")])])
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    H = T.hash_from_bytes_sha512(eng, [H_LABEL])
    half = 1 << (bits - 1)
    if transfers is None:
        rng = np.random.default_rng(n)
        transfers = rng.integers(-(half // 4), half // 4 + 1, size=(n, TRANSFERS))
        transfers[rng.random(n) < 0.5, 2] = 0                         # half of the accounts end near where ...
        transfers[:, 1] = np.where(transfers[:, 2] == 0, -transfers[:, 0] + rng.integers(-3, 4, size=n), transfers[:, 1])      # ... they began
        transfers[-1] = [half // 2, half // 2, 1]                     # the last account is out of range: 2^(bits - 1) + 1
    transfers = np.array([[int(a) for a in row] for row in transfers], dtype=object).reshape(n, TRANSFERS)
    nets = [int(sum(row)) for row in transfers]
    nt = n * TRANSFERS

    # the key and the transfers' ciphertexts
    secrets = T.scalar_random(eng, nt + 1, key)
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)
    M, bad0 = T.point_mul(eng, scalar_rows(transfers.reshape(-1)), H, ZKP_CT)
    T1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    T2, bad2 = T.point_add(eng, rY, M)
    assert not bad0.any() and not bad.any() and not bad2.any()

    # an account's ciphertext is the sum of its transfers' (the scheme is additively homomorphic)
    off = np.arange(n + 1, dtype=np.uint32) * TRANSFERS
    C1, bad = T.point_sum(eng, off, T1)
    C2, bad2 = T.point_sum(eng, off, T2)
    assert not bad.any() and not bad2.any()

    # the holder of y decrypts every account and proves it: the same witness in every proof, Y repeated as an instance point
    Z, bad = T.point_mul(eng, y, C1, ZKP_CT)
    assert not bad.any()
    Yn = np.ascontiguousarray(np.repeat(Y, n, axis=0))
    inst = np.ascontiguousarray(np.stack([Yn, Z, C1]))
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    wit = np.ascontiguousarray(np.repeat(y.reshape(1, 1, 32), n, axis=0))
    chal, resp, coms = T.prove_batch(peng, dec.statement, ts, wit, inst, B)
    say("%d accounts of %d transfers decrypted with %d-byte compact proofs" % (n, TRANSFERS, 32 + 32 * dec.statement.m))

    # the auditor: all proofs at once and one by one, then the net amounts from C2 - Z
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    T.batch_verify(peng, dec.statement, ts, inst, B, coms, resp)                 # raises on failure
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    accepted = int((T.verify_compact_batch(peng, dec.statement, ts, inst, B, chal, resp) == 0).sum())
    Z_x, _ = T.point_add(eng, Z, H)                                   # a decryption that is off by one unit is rejected: Z moves by H
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    rejected = int((T.verify_compact_batch(peng, dec.statement, ts, np.ascontiguousarray(np.stack([Yn, Z_x, C1])), B, chal, resp) != 0).sum())
    say("decryption proofs: batch verified, %d of %d accepted one by one, %d of %d shifted ones rejected" % (accepted, n, rejected, n))
    sH, bad = T.point_sub(eng, C2, Z)
    assert not bad.any()
    recovered, status = T.point_dlog(eng, H[0], sH, bits, signed=True)
    in_range = np.array([-half <= s < half for s in nets])
    ok = bool((status[in_range] == 0).all() and (status[~in_range] == 2).all()
              and all(int(k) == s for k, s, f in zip(recovered, nets, in_range) if f))
    say("net balances in [-2^%d, 2^%d) recovered: %d of %d (%d out of range), %s" % (bits - 1, bits - 1, int((status == 0).sum()), n, int((status == 2).sum()),
                                                                                 "all as transferred" if ok else "MISMATCH"))
    return {"H": H, "Y": Y, "C1": C1, "C2": C2, "Z": Z, "sH": sH, "recovered": recovered, "status": status, "nets": nets, "accepted": accepted,
            "rejected": rejected, "match": ok}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n = int(args[0]) if args else (64 if host else 4096)
    bits = int(args[1]) if len(args) > 1 else (16 if host else 32)
    if host:
        run(None, n, bits, verbose=True)
        return
    from zkp_amd.engine import Engine
    eng = Engine(0)
    try:
        run(eng, n, bits, verbose=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

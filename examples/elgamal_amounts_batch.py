#!/usr/bin/env python3
"""Verifiable decryption of N exponential-ElGamal ciphertexts of AMOUNTS below 2^bits on ristretto255, every group operation a batched call:

    the key           Y = y B                                     toolbox.basepoint_mul
    ciphertext j      (C1_j, C2_j) = (r_j B, r_j Y + a_j B)       toolbox.basepoint_mul, point_mul, point_add       a_j < 2^bits
    its decryption    Z_j = y C1_j with a proof that              toolbox.point_mul, prove_batch: a DLEQ over (B, Y ; C1_j, Z_j)
                      Y = y B  and  Z_j = y C1_j
    the auditor       batch-verifies all N decryption proofs      toolbox.batch_verify, verify_compact_batch
    the amounts       C2_j - Z_j = a_j B,  a_j = log_B            toolbox.point_sub, toolbox.basepoint_dlog

The last step is the call of include/zkp_mi355x.h section 10: baby-step / giant-step on the device (or on the host threads), instead of a table of
all 2^bits multiples of B and a row search.  A ciphertext whose plaintext is not below 2^bits comes back with status 2 (no logarithm in range).
With --host (or eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/elgamal_amounts_batch.py [N] [bits] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"ElGamal amounts example"


def scalar_rows(values) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32).copy()


def run(eng, n, bits=16, key=None, amounts=None, verbose=False):
    """N ciphertexts, their decryption proofs, the auditor's checks and the recovered amounts.  eng = an Engine, or None for the host backend.
    key (32 bytes) makes the secrets reproducible, amounts [N] fixes the plaintexts (one at or above 2^bits is reported as out of range).
    Returns a dict of what was computed and the verdicts."""
    peng = eng if eng is not None else T.HostEngine()                # (the proof calls want an object in the engine's place)
    say = print if verbose else (lambda *a: None)
    dec = T.define_proof("decryption", b"amount decryption", ["y"], ["Y", "Z", "C1"], ["B"], [("Y", [("y", "B")]), ("Z", [("y", "C1")])])
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    if amounts is None:
        amounts = np.random.default_rng(n).integers(0, 1 << bits, size=n)
    amounts = [int(a) for a in amounts]

    # the key and the ciphertexts
    secrets = T.scalar_random(eng, n + 1, key)
    y, r = secrets[:1], np.ascontiguousarray(secrets[1:])
    Y = T.basepoint_mul(eng, y)
    M = T.basepoint_mul(eng, scalar_rows(amounts))
    C1 = T.basepoint_mul(eng, r)
    rY, bad = T.point_mul(eng, r, Y, ZKP_CT)
    C2, bad2 = T.point_add(eng, rY, M)
    assert not bad.any() and not bad2.any()

    # the holder of y decrypts every ciphertext and proves it: the same witness in every proof, Y repeated as an instance point
    Z, bad = T.point_mul(eng, y, C1, ZKP_CT)
    assert not bad.any()
    Yn = np.ascontiguousarray(np.repeat(Y, n, axis=0))
    inst = np.ascontiguousarray(np.stack([Yn, Z, C1]))
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    wit = np.ascontiguousarray(np.repeat(y.reshape(1, 1, 32), n, axis=0))
    chal, resp, coms = T.prove_batch(peng, dec.statement, ts, wit, inst, B)
    say("%d ciphertexts decrypted with %d-byte compact proofs" % (n, 32 + 32 * dec.statement.m))

    # the auditor: all proofs at once and one by one, then the amounts from C2 - Z
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    T.batch_verify(peng, dec.statement, ts, inst, B, coms, resp)                 # raises on failure
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    accepted = int((T.verify_compact_batch(peng, dec.statement, ts, inst, B, chal, resp) == 0).sum())
    # a decryption that is off by one unit is rejected: Z moves by B
    Z_x, _ = T.point_add(eng, Z, B)
    ts = np.stack([T.Transcript(DOMAIN).state] * n)
    rejected = int((T.verify_compact_batch(peng, dec.statement, ts, np.ascontiguousarray(np.stack([Yn, Z_x, C1])), B, chal, resp) != 0).sum())
    say("decryption proofs: batch verified, %d of %d accepted one by one, %d of %d shifted ones rejected" % (accepted, n, rejected, n))
    aB, bad = T.point_sub(eng, C2, Z)
    assert not bad.any()
    recovered, status = T.basepoint_dlog(eng, aB, bits)
    in_range = np.array([a < (1 << bits) for a in amounts])
    ok = bool((status[in_range] == 0).all() and (status[~in_range] == 2).all()
              and all(int(k) == a for k, a, f in zip(recovered, amounts, in_range) if f))
    say("amounts below 2^%d recovered: %d of %d (%d out of range), %s" % (bits, int((status == 0).sum()), n, int((status == 2).sum()),
                                                                        "all as encrypted" if ok else "MISMATCH"))
    return {"Y": Y, "C1": C1, "C2": C2, "Z": Z, "aB": aB, "recovered": recovered, "status": status, "amounts": amounts, "accepted": accepted,
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

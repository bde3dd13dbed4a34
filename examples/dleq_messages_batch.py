#!/usr/bin/env python3
"""The reference's `create_batch_and_batch_verify` (tests/zkp.rs:115-175) for a batch of N messages on an MI355X, from product calls alone:

    define_proof! {dleq, "DLEQ Example Proof", (x), (A, B, H), (G) : A = (x * G), B = (x * H) }

The prover hashes every message to its generator H = RistrettoPoint::hash_from_bytes::<Sha512>(message) on the GPU, computes
A = x G and B = x H with the constant-time multiscalar multiplication, and proves the batch.  The verifier hashes the messages again --
it needs every H before the batch check can start -- and verifies all proofs in one batch.  Changing one message on the verifier's side
makes the batch fail.  The first four messages and secrets are the reference test's own (x = 89327492234 (i + 1)).

    python examples/dleq_messages_batch.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
REFERENCE_MESSAGES = [b"One message", b"Another message", b"A third message", b"A fourth message"]


def messages_for(n):
    return (REFERENCE_MESSAGES + [b"Message number %d of the batch" % j for j in range(4, n)])[:n]


def run(eng, messages):
    """-> (verdict of the honest batch, verdict with one message changed on the verifier's side): True = the batch verified"""
    n = len(messages)
    dleq = T.define_proof("dleq", b"DLEQ Example Proof", ["x"], ["A", "B", "H"], ["G"], [("A", [("x", "G")]), ("B", [("x", "H")])])
    st = dleq.statement
    G = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    x = np.zeros((n, 32), np.uint8)                                        # Scalar::from(89327492234) * Scalar::from(i + 1), below 2^64
    for i in range(n):
        x[i, :16] = np.frombuffer((89327492234 * (i + 1)).to_bytes(16, "little"), np.uint8)

    # prover: H per message (SHA-512 and the map on the GPU), A = x G, B = x H, prove_batchable on Transcript::new(b"DLEQTest")
    H = T.hash_from_bytes_sha512(eng, messages)
    iota = np.arange(n + 1, dtype=np.uint32)
    A, st_a = eng.msm_many(iota, x, np.zeros(n, np.uint32), G, ZKP_CT)
    B, st_b = eng.msm_many(iota, x, np.arange(n, dtype=np.uint32), H, ZKP_CT)
    assert not st_a.any() and not st_b.any()
    ts = np.stack([T.Transcript(b"DLEQTest").state] * n)
    _, resp, coms = T.prove_batch(eng, st, ts, x.reshape(n, 1, 32), np.ascontiguousarray(np.stack([A, B, H])), G)

    def verify(msgs):
        H_v = T.hash_from_bytes_sha512(eng, msgs)                         # the verifier hashes the messages itself
        ts_v = np.stack([T.Transcript(b"DLEQTest").state] * n)
        try:
            T.batch_verify(eng, st, ts_v, np.ascontiguousarray(np.stack([A, B, H_v])), G, coms, resp)
            return True
        except T.VerificationFailure:
            return False

    changed = list(messages)
    changed[n // 2] = changed[n // 2] + b"!"
    return verify(messages), verify(changed)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    eng = Engine(0)
    ok, ok_changed = run(eng, messages_for(n))
    print("batch verification of %d proofs over hashed messages: %s" % (n, "ok" if ok else "FAILED"))
    print("the same batch with message %d changed on the verifier's side: %s" % (n // 2, "ERROR: accepted" if ok_changed else "rejected"))
    eng.close()
    sys.exit(0 if ok and not ok_changed else 1)


if __name__ == "__main__":
    main()

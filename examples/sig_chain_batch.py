#!/usr/bin/env python3
"""The reference's counterparty_signature_chain (tests/sig_and_vrf_example.rs:243-281) for N PAIRS of parties at once on an MI355X, from
product calls alone:

    define_proof! {sig_proof, "Sig", (x), (A), (B) : A = (x * B) }

Two counterparties exchange signatures over stateful transcripts: when party 1 signs, party 1's transcript changes; when party 2
verifies, party 2's transcript follows.  Six rounds, the signer alternating.  Here every pair has messages of its own lengths, so
after the first round the N transcripts of a side stand at N different STROBE positions and every later append starts from a ragged
batch: append_messages(eng=...) runs them on the device, one lane per transcript, in place; prove_batch and verify_batchable_each
take the ragged batch from there.  At the end both parties' transcripts must be equal, pair by pair.

    python examples/sig_chain_batch.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"Counterparty Example"
ROUNDS = 6


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    eng = Engine(0)
    st = T.define_proof("sig_proof", b"Sig", ["x"], ["A"], ["B"], [("A", [("x", "B")])]).statement
    rng = np.random.default_rng()
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    iota = np.arange(n + 1, dtype=np.uint32)

    # a key pair per party and pair: x = Scalar::random, A = x B
    keys = []
    for _ in range(2):
        x = T.scalar_random(eng, n)
        A, _ = eng.msm_many(iota, x, np.zeros(n, np.uint32), B, ZKP_CT)
        keys.append((x.reshape(n, 1, 32), np.ascontiguousarray(A[None])))

    # trans1, trans2 = Transcript::new(domain_sep), per pair
    t0 = T.Transcript(DOMAIN).state
    trans = [np.stack([t0] * n), np.stack([t0] * n)]
    failed = False
    for r in range(ROUNDS):
        signer, verifier = r % 2, 1 - r % 2
        messages = [rng.bytes(int(k)) for k in rng.integers(8, 600, size=n)]
        x, A = keys[signer]
        # KeyPair::sign: the message goes into the signer's transcript, then prove_batchable on it
        T.append_messages(trans[signer], b"msg", messages, eng=eng)
        positions = len({bytes(b[200:203]) for b in trans[signer]})
        _, resp, coms = T.prove_batch(eng, st, trans[signer], x, A, B)
        # Signature::verify on the counterparty's transcript
        T.append_messages(trans[verifier], b"msg", messages, eng=eng)
        verdicts = T.verify_batchable_each(eng, st, trans[verifier], A, B, coms, resp)
        rejected = int((verdicts != 0).sum())
        failed |= rejected != 0
        print("round %d: party %d signed %d messages of 8..599 bytes (%d STROBE positions), party %d accepted %d"
              % (r + 1, signer + 1, n, positions, verifier + 1, n - rejected))
    equal = bool((trans[0][:, :203] == trans[1][:, :203]).all())
    print("after %d rounds: transcripts %s for %d pairs" % (ROUNDS, "equal" if equal else "DIFFER", n))
    eng.close()
    return 1 if failed or not equal else 0


if __name__ == "__main__":
    sys.exit(main())

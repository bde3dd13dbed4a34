#!/usr/bin/env python3
"""The reference's create_and_verify_sig (tests/sig_and_vrf_example.rs) for a BATCH of messages of random lengths on an MI355X, from
product calls alone:

    define_proof! {sig_proof, "Sig", (x), (A), (B) : A = (x * B) }

sign = Transcript::new(domain) ; append_message(b"msg", message) ; prove_batchable.  Messages of different lengths leave the transcripts
at different STROBE positions (a ragged batch): the appends run on the device, one lane per transcript, and the toolbox runs the proofs there with one transcript
program per position class.
Every signature is then verified one by one (verify_batchable_each) and as one batch (batch_verify), and the example's reject cases --
wrong public key, wrong message, wrong domain separator -- fail.

    python examples/sig_batch.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"My Sig Application"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    eng = Engine(0)
    st = T.define_proof("sig_proof", b"Sig", ["x"], ["A"], ["B"], [("A", [("x", "B")])]).statement
    rng = np.random.default_rng()
    messages = [rng.bytes(int(k)) for k in rng.integers(8, 600, size=n)]
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()

    # one key pair per signer: x = Scalar::random (sig_and_vrf_example.rs:49), A = x B
    x = T.scalar_random(eng, n)
    A, _ = eng.msm_many(np.arange(n + 1, dtype=np.uint32), x, np.zeros(n, np.uint32), B, ZKP_CT)

    # KeyPair::sign: the message goes into the transcript, then prove_batchable
    ts = T.append_messages(DOMAIN, b"msg", messages, eng=eng)
    positions = len({bytes(r[200:203]) for r in ts})
    _, resp, coms = T.prove_batch(eng, st, ts, x.reshape(n, 1, 32), np.ascontiguousarray(A[None]), B)
    print("signed %d messages of 8..599 bytes (%d STROBE positions): %d-byte batchable signatures" % (n, positions, 32 + 32 * st.m))

    def verify_each(msgs, A_v, domain):
        """Signature::verify for every signature -> verdicts, 0 = accepted"""
        return T.verify_batchable_each(eng, st, T.append_messages(domain, b"msg", msgs, eng=eng), np.ascontiguousarray(A_v[None]), B, coms, resp)

    def verify_batch(msgs, A_v, domain):
        try:
            T.batch_verify(eng, st, T.append_messages(domain, b"msg", msgs, eng=eng), np.ascontiguousarray(A_v[None]), B, coms, resp)
            return True
        except T.VerificationFailure:
            return False

    ok = verify_each(messages, A, DOMAIN)
    batch_ok = verify_batch(messages, A, DOMAIN)
    print("verify: %d of %d accepted one by one; the batch %s" % (int((ok == 0).sum()), n, "verifies" if batch_ok else "FAILS"))
    shift = np.roll(np.arange(n), 1)                                 # everybody gets the neighbour's key / message
    failed = ok.any() or not batch_ok
    for what, msgs, A_v, domain in (("wrong public key", messages, A[shift], DOMAIN),
                                    ("wrong message", [messages[j] for j in shift], A, DOMAIN),
                                    ("wrong domain separator", messages, A, b"A different application")):
        verdicts = verify_each(msgs, A_v, domain)
        batch = verify_batch(msgs, A_v, domain)
        print("%-24s %d of %d rejected; the batch %s" % (what + ":", int((verdicts != 0).sum()), n, "verifies" if batch else "fails"))
        failed |= not verdicts.all() or batch
    eng.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

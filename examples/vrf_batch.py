#!/usr/bin/env python3
"""The reference's VRF example (tests/sig_and_vrf_example.rs) for a BATCH of messages on an MI355X, from product calls alone:

    define_proof! {vrf_proof, "VRF", (x), (A, G, H), (B) : A = (x * B), G = (x * H) }

For each message: H = hash_to_group(function transcript) -- merlin's challenge_bytes(b"output", 64) then
RistrettoPoint::from_uniform_bytes, on the GPU --, the VRF output G = x H (constant-time multiscalar multiplication), and a compact
proof that log_B(A) = log_H(G).  Unlike examples/dleq_batch.py, nobody knows log_B(H) here: H comes out of a hash.  Then every
proof is verified, and the example's reject cases (wrong public key, wrong output, wrong domain separator, wrong message) fail.

    python examples/vrf_batch.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"My VRF Application"


def function_transcripts(eng, messages, domain=DOMAIN):
    """Transcript::new(domain) + append_message_example(message) (sig_and_vrf_example.rs:33-35), one per message, appended on the device"""
    return T.append_messages(domain, b"msg", messages, eng=eng)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    eng = Engine(0)
    vrf = T.define_proof("vrf_proof", b"VRF", ["x"], ["A", "G", "H"], ["B"], [("A", [("x", "B")]), ("G", [("x", "H")])])
    st = vrf.statement
    messages = [b"Test Message %d" % j for j in range(n)]
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()

    # one key pair per message (a batch of VRF evaluations for many users): x = Scalar::random (sig_and_vrf_example.rs:49), A = x B
    x = T.scalar_random(eng, n)
    iota = np.arange(n + 1, dtype=np.uint32)
    A, _ = eng.msm_many(iota, x, np.zeros(n, np.uint32), B, ZKP_CT)

    # VRF evaluation: H = hash_to_group(function transcript), G = x H, proof on Transcript::new(domain)
    H = T.hash_to_group(eng, function_transcripts(eng, messages))
    G, _ = eng.msm_many(iota, x, np.arange(n, dtype=np.uint32), H, ZKP_CT)
    proof_ts = np.stack([T.Transcript(DOMAIN).state] * n)
    chal, resp, _ = T.prove_batch(eng, st, proof_ts, x.reshape(n, 1, 32), np.ascontiguousarray(np.stack([A, G, H])), B)
    print("evaluated the VRF on %d messages: %d-byte outputs, %d-byte compact proofs" % (n, 32, 32 + 32 * st.m))

    def verify(msgs, A_v, G_v, domain):
        """VrfOutput::verify (sig_and_vrf_example.rs): the verifier hashes the message itself -> verdicts, 0 = accepted"""
        H_v = T.hash_to_group(eng, function_transcripts(eng, msgs))
        ts = np.stack([T.Transcript(domain).state] * n)
        return T.verify_compact_batch(eng, st, ts, np.ascontiguousarray(np.stack([A_v, G_v, H_v])), B, chal, resp)

    ok = verify(messages, A, G, DOMAIN)
    print("verify: %d of %d accepted" % (int((ok == 0).sum()), n))
    shift = np.roll(np.arange(n), 1)                                 # everybody gets the neighbour's key / output / message
    for what, verdicts in (("wrong public key", verify(messages, A[shift], G, DOMAIN)),
                           ("wrong output", verify(messages, A, G[shift], DOMAIN)),
                           ("wrong domain separator", verify(messages, A, G, b"A different application")),
                           ("wrong message", verify([messages[j] for j in shift], A, G, DOMAIN))):
        print("%-24s %d of %d rejected" % (what + ":", int((verdicts != 0).sum()), n))
    eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The reference's KeyPair::from plus KeyPair::vrf (tests/sig_and_vrf_example.rs:56-60, 103-125) for N DISTINCT keys, every group
operation a batched product call:

    sk_j = Scalar::random                                   toolbox.scalar_random
    pk_j = &sk_j * &RISTRETTO_BASEPOINT_TABLE   (:58)       toolbox.basepoint_mul      one launch, the context's own table of B
    H_j  = hash_to_group(function transcript)   (:36-40)    toolbox.hash_to_group
    G_j  = &H_j * &sk_j                         (:112)      toolbox.point_mul          one launch, constant time
    proof that log_B(pk_j) = log_H(G_j)         (:114-123)  toolbox.prove_batch / verify_compact_batch

No CSR index arrays and no Engine.msm_many: the two multiplications are the calls of include/zkp_mi355x.h section 8.  With --host (or
eng = None in run()) everything runs on the host backend and needs no GPU.

    python examples/keygen_vrf_batch.py [N] [--host]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
DOMAIN = b"My VRF Application"


def run(eng, n, key=None, verbose=False):
    """N key pairs, N VRF evaluations with their proofs, the verification and the example's reject cases.  eng = an Engine, or None for
    the host backend.  key (32 bytes) makes the secret keys reproducible.  Returns {"pk", "G", "accepted", "rejected": {case: count}}."""
    peng = eng if eng is not None else T.HostEngine()                # (the proof calls want an object in the engine's place)
    say = print if verbose else (lambda *a: None)
    vrf = T.define_proof("vrf_proof", b"VRF", ["x"], ["A", "G", "H"], ["B"], [("A", [("x", "B")]), ("G", [("x", "H")])])
    st = vrf.statement
    messages = [b"Test Message %d" % j for j in range(n)]
    B = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()

    # KeyPair::from(SecretKey::new(rng)): one key pair per user
    sk = T.scalar_random(eng, n, key)
    pk = T.basepoint_mul(eng, sk)

    # KeyPair::vrf: H = hash_to_group(function transcript), G = H * sk, proof on Transcript::new(domain)
    H = T.hash_to_group(eng, T.append_messages(DOMAIN, b"msg", messages, eng=eng))
    G, bad = T.point_mul(eng, sk, H, ZKP_CT)
    assert not bad.any()                                             # (a hash output always decodes)
    proof_ts = np.stack([T.Transcript(DOMAIN).state] * n)
    chal, resp, _ = T.prove_batch(peng, st, proof_ts, sk.reshape(n, 1, 32), np.ascontiguousarray(np.stack([pk, G, H])), B)
    say("%d key pairs, %d VRF outputs with %d-byte compact proofs" % (n, n, 32 + 32 * st.m))

    def verify(msgs, pk_v, G_v, domain):
        """VrfOutput::verify: the verifier hashes the message itself -> verdicts, 0 = accepted"""
        H_v = T.hash_to_group(eng, T.append_messages(DOMAIN, b"msg", msgs, eng=eng))
        ts = np.stack([T.Transcript(domain).state] * n)
        return T.verify_compact_batch(peng, st, ts, np.ascontiguousarray(np.stack([pk_v, G_v, H_v])), B, chal, resp)

    accepted = int((verify(messages, pk, G, DOMAIN) == 0).sum())
    say("verify: %d of %d accepted" % (accepted, n))
    shift = np.roll(np.arange(n), 1)                                 # everybody gets the neighbour's key / output / message
    rejected = {}
    for what, verdicts in (("wrong public key", verify(messages, pk[shift], G, DOMAIN)),
                           ("wrong output", verify(messages, pk, G[shift], DOMAIN)),
                           ("wrong domain separator", verify(messages, pk, G, b"A different application")),
                           ("wrong message", verify([messages[j] for j in shift], pk, G, DOMAIN))):
        rejected[what] = int((verdicts != 0).sum())
        say("%-24s %d of %d rejected" % (what + ":", rejected[what], n))
    return {"sk": sk, "pk": pk, "H": H, "G": G, "accepted": accepted, "rejected": rejected}


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host = "--host" in sys.argv[1:]
    n = int(args[0]) if args else (64 if host else 4096)
    if host:
        run(None, n, verbose=True)
        return
    from zkp_amd.engine import Engine
    eng = Engine(0)
    try:
        run(eng, n, verbose=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

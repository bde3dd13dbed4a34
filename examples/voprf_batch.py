#!/usr/bin/env python3
"""A blinded evaluation (the best-known deployment of the reference's DLEQ proof, tests/zkp.rs:28) for a batch of N inputs on an
MI355X, from product calls alone:

    define_proof! {dleq, "DLEQ Example Proof", (x), (A, B, H), (G) : A = (x * G), B = (x * H) }

with x = the server's key k, A = Y = k G, H = the blinded element M_i and B = Z_i = k M_i.

    client   T_i = hash_from_bytes::<Sha512>(input_i);  r_i = Scalar::random;  M_i = r_i T_i       (constant-time multiplication)
    server   Z_i = k M_i and a proof that log_G(Y) = log_{M_i}(Z_i), one per element
    client   batch-verifies the proofs, then unblinds: N_i = r_i^-1 Z_i  (Scalar::invert for the batch) -- which is k T_i

The example checks N_i against k T_i computed directly, and that the batch fails once one Z_i is replaced.

    python examples/voprf_batch.py [N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from zkp_amd import toolbox as T
from zkp_amd.engine import Engine, ZKP_CT

BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


def run(eng, n):
    """-> {"verified": the honest batch verifies, "unblinded": every N_i equals k T_i, "rejected_tampered": the batch with one Z_i
    replaced fails}"""
    dleq = T.define_proof("dleq", b"DLEQ Example Proof", ["x"], ["A", "B", "H"], ["G"], [("A", [("x", "G")]), ("B", [("x", "H")])])
    st = dleq.statement
    G = np.frombuffer(BASEPOINT, np.uint8).reshape(1, 32).copy()
    each = np.arange(n, dtype=np.uint32)
    zeros = np.zeros(n, np.uint32)

    def mul(scalars, points, pidx):
        out, status = eng.msm_many(np.arange(len(scalars) + 1, dtype=np.uint32), scalars, pidx, points, ZKP_CT)
        assert not status.any()
        return out

    # client: hash the inputs to the group, draw the blinds, blind
    inputs = [b"input number %d" % j for j in range(n)]
    Tp = T.hash_from_bytes_sha512(eng, inputs)
    r = T.scalar_random(eng, n)
    M = mul(r, Tp, each)

    # server: one key for the batch, Y = k G, Z_i = k M_i, one DLEQ proof per element
    k = T.scalar_random(eng, 1)
    kk = np.repeat(k, n, axis=0)
    Y = mul(k, G, zeros[:1])
    Z = mul(kk, M, each)
    inst = np.ascontiguousarray(np.stack([np.repeat(Y, n, axis=0), Z, M]))
    ts = np.stack([T.Transcript(b"VOPRF evaluation").state] * n)
    _, resp, coms = T.prove_batch(eng, st, ts, kk.reshape(n, 1, 32), inst, G)

    # client: verify the batch, unblind with r^-1
    def verify(Z_v):
        ts_v = np.stack([T.Transcript(b"VOPRF evaluation").state] * n)
        try:
            T.batch_verify(eng, st, ts_v, np.ascontiguousarray(np.stack([np.repeat(Y, n, axis=0), Z_v, M])), G, coms, resp)
            return True
        except T.VerificationFailure:
            return False

    verified = verify(Z)
    r_inv = T.scalar_invert(eng, r)
    N = mul(r_inv, Z, each)
    unblinded = bool((N == mul(kk, Tp, each)).all())
    tampered = Z.copy()
    tampered[n // 2] = M[n // 2]                                           # a valid point that is not k M
    return {"verified": verified, "unblinded": unblinded, "rejected_tampered": not verify(tampered)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    eng = Engine(0)
    res = run(eng, n)
    eng.close()
    print("blinded evaluation of %d inputs: proofs %s, unblinded outputs %s, batch with one Z replaced %s" % (
        n, "verify" if res["verified"] else "FAIL", "equal k T" if res["unblinded"] else "DIFFER", "rejected" if res["rejected_tampered"] else "ACCEPTED"))
    return 0 if all(res.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

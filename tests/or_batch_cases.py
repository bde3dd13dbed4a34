"""Inputs shared by the tests of the batchable OR-proofs (tests/test_host_or_batch*.py, tests/test_gpu_or_batch*.py): the cases of
tests/or_proof_cases.py with the model's commitments (tests/or_batch_model.py), the three weight patterns, the coefficient vector as numpy
rows, the tamperings of or_proof_cases plus four on the commitments, and the footprint cases of the two new headers."""
import functools

import numpy as np

from tests import or_batch_model as BM
from tests import or_proof_cases as C
from zkp_amd import toolbox as T

L = C.L
WEIGHT_PATTERNS = ("random", "zero", "ones")


def _lists(c, j, inst=None):
    """proof j's inst [k][ni] and common [ns] as byte strings"""
    inst = c.inst if inst is None else inst
    return ([[inst[b, v, j].tobytes() for v in range(c.st.ni)] for b in range(c.k)], [c.common[p].tobytes() for p in range(c.st.ns)])


def _proof_lists(c, j, coms, chal, resp):
    return ([[coms[j, b, i].tobytes() for i in range(c.st.nc)] for b in range(c.k)], [chal[j, b].tobytes() for b in range(c.k)],
            [[resp[j, b, i].tobytes() for i in range(c.st.m)] for b in range(c.k)])


@functools.lru_cache(maxsize=None)
def _model(name: str, k: int):
    c = C.case(name, k)
    stmt = C.model_statement(name)
    ts, coms, chal, resp = [], [], [], []
    for j in range(C.MODEL_N):
        t = C.blob_to_model(c.transcripts[j])
        inst, com = _lists(c, j)
        cm, ch, rs = BM.prove(t, stmt, k, [c.secrets[j, i].tobytes() for i in range(c.st.m)], int(c.real[j]), inst, com, c.entropy[j].tobytes())
        ts.append(C.model_to_blob(t))
        coms.append(b"".join(b"".join(row) for row in cm))
        chal.append(b"".join(ch))
        resp.append(b"".join(b"".join(row) for row in rs))
    return (np.stack(ts).tobytes(), b"".join(coms), b"".join(chal), b"".join(resp))


def model(name: str, k: int, n: int = C.MODEL_N):
    """the model's (transcripts [n][208], commitments [n][k][nc][32], challenges [n][k][32], responses [n][k][m][32]), n <= MODEL_N"""
    ts, coms, chal, resp = _model(name, k)
    st = C.statement(name)
    N = C.MODEL_N
    return (np.frombuffer(ts, np.uint8).reshape(N, 208)[:n].copy(), np.frombuffer(coms, np.uint8).reshape(N, k, st.nc, 32)[:n].copy(),
            np.frombuffer(chal, np.uint8).reshape(N, k, 32)[:n].copy(), np.frombuffer(resp, np.uint8).reshape(N, k, st.m, 32)[:n].copy())


def model_verify(name, c, j, coms, chal, resp, inst=None) -> bool:
    t = C.blob_to_model(c.transcripts[j])
    i, com = _lists(c, j, inst)
    return BM.verify_batchable(t, C.model_statement(name), c.k, i, com, *_proof_lists(c, j, coms, chal, resp))


def model_batch_verify(name, c, coms, chal, resp, weights16, inst=None) -> bool:
    """the model's whole batch check, group sum included (pure Python: small batches only)"""
    ts = [C.blob_to_model(c.transcripts[j]) for j in range(c.n)]
    lists = [_lists(c, j, inst) for j in range(c.n)]
    proofs = [_proof_lists(c, j, coms, chal, resp) for j in range(c.n)]
    return BM.batch_verify(ts, C.model_statement(name), c.k, [x[0] for x in lists], lists[0][1], [p[0] for p in proofs], [p[1] for p in proofs],
                           [p[2] for p in proofs], weight_ints(weights16))


def weights(pattern: str, n: int, k: int, nc: int, seed: int = 7) -> np.ndarray:
    """weights16 uint8 [n][k][nc][16]: random, all zero, or all 0xff (the largest u128)"""
    if pattern == "zero":
        return np.zeros((n, k, nc, 16), np.uint8)
    if pattern == "ones":
        return np.full((n, k, nc, 16), 0xff, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, size=(n, k, nc, 16), dtype=np.uint8)


def weight_ints(w16: np.ndarray):
    n, k, nc, _ = w16.shape
    flat = w16.reshape(-1, 16)
    vals = [int.from_bytes(row.tobytes(), "little") for row in flat]
    return [[[vals[(j * k + b) * nc + c] for c in range(nc)] for b in range(k)] for j in range(n)]


def _ints(a: np.ndarray):
    """uint8 [...][32] -> nested lists of Python integers"""
    if a.ndim == 1:
        return int.from_bytes(a.tobytes(), "little")
    return [_ints(x) for x in a]


def model_coeffs(name, k, chal, resp, w16) -> np.ndarray:
    """BM.batch_coeffs as uint8 [ns + n k (ni + nc)][32]"""
    n = len(chal)
    out = BM.batch_coeffs(C.model_statement(name), k, n, _ints(chal), _ints(resp), weight_ints(w16))
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in out), np.uint8).reshape(len(out), 32).copy()


def commitment_tamperings(c, coms: np.ndarray):
    """[(what, commitments, victim)]: ONE proof's commitments spoiled (k >= 2 or nc >= 2, n >= 16)"""
    out = []

    def add(what, victim, f):
        cm = coms.copy()
        f(cm, victim)
        out.append((what, cm, victim))

    def swap(cm, j):
        flat = cm[j].reshape(-1, 32)
        flat[0], flat[-1] = flat[-1].copy(), flat[0].copy()

    add("a commitment replaced by another valid point", 8, lambda cm, j: cm.__setitem__((j, 0, 0), cm[j + 1, 0, 0]))
    add("a commitment replaced by 32 zero bytes", 9, lambda cm, j: cm.__setitem__((j, c.k - 1, 0), 0))
    add("a commitment replaced by a non-decoding encoding", 10, lambda cm, j: cm.__setitem__((j, 0, c.st.nc - 1), C.NON_DECODING))
    add("two commitments of one proof swapped", 11, swap)
    return out


def tamperings(c, coms, chal, resp):
    """[(what, commitments, challenges, responses, inst, victim)]: or_proof_cases' seven and the four on the commitments"""
    out = [(what, coms, ch, rs, inst, victim) for what, ch, rs, inst, victim in C.tamperings(c, chal, resp)]
    return out + [(what, cm, chal, resp, c.inst, victim) for what, cm, victim in commitment_tamperings(c, coms)]


# ---- the footprint cases: every call of the two new headers that takes a non-const pointer --------------------------------------------------
FOOTPRINT = C.FOOTPRINT
FOOTPRINT_FUNCTIONS = {
    "host": ("zkp_or_prove_batchable", "zkp_or_verify_batchable", "zkp_or_batch_verify"),
    "dev": ("zkp_or_prove_batchable_dev", "zkp_or_verify_batchable_dev", "zkp_or_batch_verify_dev"),
    "batch": ("zkp_or_prove_batchable_batch", "zkp_or_verify_batchable_batch", "zkp_or_batch_verify_batch", "zkp_or_batch_verify_locate",
              "zkp_or_batch_verify_coeffs")}


@functools.lru_cache(maxsize=None)
def _footprint_reference(n: int):
    """(case, advanced transcripts, commitments, challenges, responses, weights16, coefficient rows): the model's proofs up to MODEL_N, the
    host backend's beyond; the coefficients are the model's either way"""
    name, k = FOOTPRINT
    c = C.case(name, k, n)
    if n <= C.MODEL_N:
        ts, coms, chal, resp = model(name, k, n)
    else:
        ts = c.transcripts.copy()
        coms, chal, resp, status = T.or_prove_batchable(None, c.st, ts, c.secrets, c.real, c.inst, c.common, c.entropy)
        assert not status.any()
    w = weights("random", n, k, c.st.nc)
    return c, ts, coms, chal, resp, w, model_coeffs(name, k, chal, resp, w)


def footprint_cases(form: str):
    """tests.footprint_cases.Case objects of form "host", "dev" or "batch" (ctx == NULL, 1 and 3 threads): valid proofs, so the transcripts
    are exact in/out operands and every verdict is 0"""
    import ctypes

    from tests import footprint_cases as F
    name, k = FOOTPRINT
    out = []
    for n in F.TRANSCRIPT_SIZES:
        for threads in ((1, 3) if form == "batch" else (0,)):
            def build(fn, n=n, threads=threads):
                c, ts, coms, chal, resp, w, coeffs = _footprint_reference(n)
                head = [None, c.st._h, k, n] if form == "batch" else [F.CTX, ctypes.byref(C.fused_statement(name).c), k, n]
                t = F.INOUT("transcripts", c.transcripts, ts)
                inst, com = F.IN("inst", c.inst.reshape(-1, 32)), F.IN("common", c.common)
                tail = [threads] if form == "batch" else []
                if "prove" in fn:
                    return head + [t, F.IN("secrets", c.secrets.reshape(-1, 32)), F.IN("real", c.real), inst, com, F.IN("entropy", c.entropy, align=16)] + tail + [
                        F.OUT("commitments", coms.reshape(-1, 32)), F.OUT("challenges", chal.reshape(-1, 32)), F.OUT("responses", resp.reshape(-1, 32)),
                        F.OUT("status", np.zeros(n, np.uint8))]
                proof = [t, inst, com, F.IN("commitments", coms.reshape(-1, 32)), F.IN("challenges", chal.reshape(-1, 32)), F.IN("responses", resp.reshape(-1, 32))]
                if "verify_batchable" in fn:
                    return head + proof + tail + [F.OUT("results", np.zeros(n, np.uint8))]
                proof.append(F.IN("weights16", w.reshape(-1, 16)))
                if fn == "zkp_or_batch_verify":
                    return head + proof + [F.OUT("verdict", np.zeros(1, np.int32)), F.OUT("debug_scalars", coeffs)]
                if fn == "zkp_or_batch_verify_dev":
                    return head + proof + [F.OUT("verdict", np.zeros(1, np.uint32))]
                if fn == "zkp_or_batch_verify_locate":
                    return head + proof + tail + [F.OUT("results", np.zeros(n, np.uint8))]
                if fn == "zkp_or_batch_verify_coeffs":
                    return head + proof + tail + [F.OUT("coeffs", coeffs)]
                return head + proof + tail
            variant = "t%d" % threads if form == "batch" else ""
            for fn in FOOTPRINT_FUNCTIONS[form]:
                out.append(F.Case(fn, form, n, variant, functools.partial(build, fn)))
    return out

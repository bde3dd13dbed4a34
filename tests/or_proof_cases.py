"""Inputs shared by the OR-proof tests (tests/test_host_or_proof*.py, tests/test_gpu_or_proof*.py): three statements, one input generator
and the model's proofs (tests/or_proof_model.py over oracle.model), computed once per (statement, k) for MODEL_N proofs and cut down for
smaller batches.

S1  a Schnorr key  X = x B            m = 1, nc = 1, ns = 1: a ring signature over k keys
S2  dleq_module()  A = x G, B = x H   nc = 2, H an instance point
S3  a Pedersen opening  C = v G + r H m = 2, one two-term constraint, ns = 2
real[j] = j mod k unless a test says otherwise; the entropy is fixed, so proofs are deterministic."""
import functools

import numpy as np

from oracle import model as M
from tests import or_proof_model as OM
from zkp_amd import toolbox as T
from zkp_amd.engine import ZKP_CT

L = T.L
MODEL_N = 65
SIZES = (1, 33, 65, 257)          # TRANSCRIPT_SIZES
KS = (1, 2, 3, 5)
NAMES = ("S1", "S2", "S3")


@functools.lru_cache(maxsize=None)
def statement(name: str) -> T.Statement:
    if name == "S2":
        return T.dleq_module().statement
    if name == "S1":
        st = T.Statement(b"Schnorr key")
        x = st.add_secret(b"x")
        X = st.add_point(b"X", False)
        B = st.add_point(b"B", True)
        st.constrain(X, [(x, B)])
        return st
    st = T.Statement(b"Pedersen opening")
    v, r = st.add_secret(b"v"), st.add_secret(b"r")
    C = st.add_point(b"C", False)
    G, H = st.add_point(b"G", True), st.add_point(b"H", True)
    st.constrain(C, [(v, G), (r, H)])
    return st


def model_statement(name: str):
    st = statement(name)
    return (st.proof_label, list(st.secrets), list(st.points), list(st.constraints))


@functools.lru_cache(maxsize=None)
def fused_statement(name: str):
    """(kept for the process: a call holds pointers into it)"""
    from zkp_amd.engine import FusedStatement
    st = statement(name)
    return FusedStatement(st.proof_label, st.secrets, st.points, st.constraints)


def scalars(seed: int, shape) -> np.ndarray:
    """canonical scalars uint8 [*shape][32]"""
    n = int(np.prod(shape))
    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 64), dtype=np.uint8)
    return T.scalar_from_wide(None, raw).reshape(tuple(shape) + (32,))


def _mul(s, p):
    out, bad = T.point_mul(None, np.ascontiguousarray(s), np.ascontiguousarray(p), ZKP_CT)
    assert not bad.any()
    return out


class Case:
    """transcripts [N][208], secrets [N][m][32], real [N], inst [k][ni][N][32], common [ns][32], entropy [N][32]"""

    def __init__(self, name, k, n, real=None, ragged=False):
        st = statement(name)
        self.name, self.k, self.n, self.st = name, k, n, st
        seed = 1000 * NAMES.index(name) + 10 * k
        self.real = (np.arange(n) % k).astype(np.uint8) if real is None else np.asarray(real, np.uint8)
        self.secrets = scalars(seed + 1, (n, st.m))
        self.entropy = np.random.default_rng(seed + 2).integers(0, 256, size=(n, 32), dtype=np.uint8)
        common = T.basepoint_mul(None, scalars(seed + 3, (st.ns,)))
        # every branch starts from random valid points; the real branch's left-hand sides are then computed from the witness
        inst = T.basepoint_mul(None, scalars(seed + 4, (k * st.ni * n,)).reshape(-1, 32)).reshape(k, st.ni, n, 32).copy()
        j = np.arange(n)
        if name == "S1":
            inst[self.real, 0, j] = _mul(self.secrets[:, 0], np.tile(common[0], (n, 1)))
        elif name == "S2":          # instance ranks: A = 0, B = 1, H = 2
            inst[self.real, 0, j] = _mul(self.secrets[:, 0], np.tile(common[0], (n, 1)))
            inst[self.real, 1, j] = _mul(self.secrets[:, 0], inst[self.real, 2, j])
        else:
            a = _mul(self.secrets[:, 0], np.tile(common[0], (n, 1)))
            b = _mul(self.secrets[:, 1], np.tile(common[1], (n, 1)))
            s, bad = T.point_add(None, a, b)
            assert not bad.any()
            inst[self.real, 0, j] = s
        self.inst, self.common = np.ascontiguousarray(inst), np.ascontiguousarray(common)
        ts = np.stack([T.Transcript(b"OR proof tests").state] * n)
        if ragged:                  # messages of different lengths first: a mix of STROBE positions
            T.append_messages(ts, b"msg", [bytes(range(j % 37)) * (1 + j % 5) for j in range(n)])
        self.transcripts = np.ascontiguousarray(ts)

    def cut(self, n):
        """the first n proofs"""
        c = object.__new__(Case)
        c.name, c.k, c.n, c.st = self.name, self.k, n, self.st
        c.real, c.secrets, c.entropy = self.real[:n].copy(), self.secrets[:n].copy(), self.entropy[:n].copy()
        c.inst, c.common = np.ascontiguousarray(self.inst[:, :, :n]), self.common.copy()
        c.transcripts = self.transcripts[:n].copy()
        return c

    def prove(self, eng, threads=0, entropy="fixed"):
        ts = self.transcripts.copy()
        ent = self.entropy if isinstance(entropy, str) else entropy
        chal, resp, status = T.or_prove(eng, self.st, ts, self.secrets, self.real, self.inst, self.common, ent, threads)
        return ts, chal, resp, status

    def verify(self, eng, chal, resp, threads=0, inst=None):
        ts = self.transcripts.copy()
        res = T.or_verify(eng, self.st, ts, self.inst if inst is None else inst, self.common, chal, resp, threads)
        return ts, res


@functools.lru_cache(maxsize=None)
def case(name: str, k: int, n: int = MODEL_N) -> Case:
    """the case of (statement, k) over n proofs; the tests copy what they change"""
    if n < MODEL_N:
        return case(name, k, MODEL_N).cut(n)
    return Case(name, k, n)


def blob_to_model(blob: np.ndarray) -> M.Transcript:
    t = object.__new__(M.Transcript)
    s = object.__new__(M.Strobe128)
    s.state = bytearray(blob[:200].tobytes())
    s.pos, s.pos_begin, s.cur_flags = int(blob[200]), int(blob[201]), int(blob[202])
    t.strobe = s
    return t


def model_to_blob(t: M.Transcript) -> np.ndarray:
    s = t.strobe
    return np.frombuffer(bytes(s.state) + bytes([s.pos, s.pos_begin, s.cur_flags, 0, 0, 0, 0, 0]), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def _model(name: str, k: int):
    c = case(name, k)
    stmt = model_statement(name)
    ts, chal, resp = [], [], []
    for j in range(MODEL_N):
        t = blob_to_model(c.transcripts[j])
        inst = [[c.inst[b, v, j].tobytes() for v in range(c.st.ni)] for b in range(k)]
        com = [c.common[p].tobytes() for p in range(c.st.ns)]
        ch, rs = OM.prove(t, stmt, k, [c.secrets[j, i].tobytes() for i in range(c.st.m)], int(c.real[j]), inst, com, c.entropy[j].tobytes())
        ts.append(model_to_blob(t))
        chal.append(b"".join(ch))
        resp.append(b"".join(b"".join(row) for row in rs))
    return (np.stack(ts).tobytes(), b"".join(chal), b"".join(resp))


def model(name: str, k: int, n: int = MODEL_N):
    """the model's (transcripts [n][208], challenges [n][k][32], responses [n][k][m][32]) for case(name, k, n), n <= MODEL_N"""
    ts, chal, resp = _model(name, k)
    m = statement(name).m
    return (np.frombuffer(ts, np.uint8).reshape(MODEL_N, 208)[:n].copy(), np.frombuffer(chal, np.uint8).reshape(MODEL_N, k, 32)[:n].copy(),
            np.frombuffer(resp, np.uint8).reshape(MODEL_N, k, m, 32)[:n].copy())


def model_verify(name: str, c: Case, j: int, chal, resp, inst=None) -> bool:
    inst = c.inst if inst is None else inst
    t = blob_to_model(c.transcripts[j])
    return OM.verify(t, model_statement(name), c.k, [[inst[b, v, j].tobytes() for v in range(c.st.ni)] for b in range(c.k)],
                     [c.common[p].tobytes() for p in range(c.st.ns)], [chal[j, b].tobytes() for b in range(c.k)],
                     [[resp[j, b, i].tobytes() for i in range(c.st.m)] for b in range(c.k)])


SCALAR_L = np.frombuffer(L.to_bytes(32, "little"), np.uint8)


def add_l(row: np.ndarray) -> np.ndarray:
    """value + l as 32 bytes (the values here are below 2^252, so it fits)"""
    return np.frombuffer((int.from_bytes(row.tobytes(), "little") + L).to_bytes(32, "little"), np.uint8).copy()


# an encoding that does not decode: s = 1 is odd ("negative"), which RFC 9496 decoding refuses; it is not the identity's 32 zero bytes
NON_DECODING = np.frombuffer((1).to_bytes(32, "little"), np.uint8)


def _bump(row: np.ndarray) -> np.ndarray:
    return np.frombuffer(((int.from_bytes(row.tobytes(), "little") + 1) % L).to_bytes(32, "little"), np.uint8).copy()


def tamperings(c: Case, chal: np.ndarray, resp: np.ndarray):
    """The rejection matrix: [(what, challenges, responses, inst, victim)], each a copy of the valid proofs of case c (k >= 2, n >= 16) with
    ONE proof spoiled; every other proof of the batch must stay accepted."""
    out = []

    def add(what, victim, f):
        ch, rs, inst = chal.copy(), resp.copy(), c.inst.copy()
        f(ch, rs, inst, victim)
        out.append((what, ch, rs, inst, victim))

    def swap(ch, rs, inst, j):
        ch[j, 0], ch[j, 1] = ch[j, 1].copy(), ch[j, 0].copy()

    def other_point(ch, rs, inst, j):
        inst[c.k - 1, 0, j] = inst[0, 0, j + 1]

    add("a bumped response", 1, lambda ch, rs, inst, j: rs.__setitem__((j, c.k - 1, 0), _bump(rs[j, c.k - 1, 0])))
    add("a bumped challenge", 2, lambda ch, rs, inst, j: ch.__setitem__((j, 0), _bump(ch[j, 0])))
    add("two branches' challenges swapped", 3, swap)
    add("a response of value + l", 4, lambda ch, rs, inst, j: rs.__setitem__((j, 0, 0), add_l(rs[j, 0, 0])))
    add("an instance point replaced by another valid point", 5, other_point)
    add("an instance point replaced by 32 zero bytes", 6, lambda ch, rs, inst, j: inst.__setitem__((0, 0, j), 0))
    add("an instance point replaced by a non-decoding encoding", 7, lambda ch, rs, inst, j: inst.__setitem__((1, 0, j), NON_DECODING))
    return out


# ---- the footprint cases: every call of the two OR headers that takes a non-const pointer, over tests/footprint_cases.py's check ------------
FOOTPRINT = ("S2", 3)
FOOTPRINT_FUNCTIONS = {"host": ("zkp_or_prove", "zkp_or_verify"), "dev": ("zkp_or_prove_dev", "zkp_or_verify_dev"),
                       "batch": ("zkp_or_prove_batch", "zkp_or_verify_batch")}


@functools.lru_cache(maxsize=None)
def _footprint_reference(n: int):
    """(case, advanced transcripts, challenges, responses): the model's bytes up to MODEL_N proofs, the host backend's beyond"""
    name, k = FOOTPRINT
    if n <= MODEL_N:
        return (case(name, k, n),) + model(name, k, n)
    c = case(name, k, n)
    ts, chal, resp, status = c.prove(None)
    assert not status.any()
    return c, ts, chal, resp


def footprint_cases(form: str):
    """tests.footprint_cases.Case objects of form "host" (host pointers), "dev" (device pointers) or "batch" (the toolbox calls, ctx == NULL,
    1 and 3 threads): valid proofs, so the transcripts are exact in/out operands.  32-byte rows and transcripts at 16-byte alignment on the
    device, real / status / results at any."""
    import ctypes

    from tests import footprint_cases as F
    name, k = FOOTPRINT
    out = []
    for n in F.TRANSCRIPT_SIZES:
        for threads in ((1, 3) if form == "batch" else (0,)):
            def build(n=n, threads=threads, prove=True):
                c, ts, chal, resp = _footprint_reference(n)
                head = [None, c.st._h, k, n] if form == "batch" else [F.CTX, ctypes.byref(fused_statement(name).c), k, n]
                t = F.INOUT("transcripts", c.transcripts, ts)
                inst, com = F.IN("inst", c.inst.reshape(-1, 32)), F.IN("common", c.common)
                tail = [threads] if form == "batch" else []
                if prove:
                    return head + [t, F.IN("secrets", c.secrets.reshape(-1, 32)), F.IN("real", c.real), inst, com, F.IN("entropy", c.entropy, align=16)] + tail + [
                        F.OUT("challenges", chal.reshape(-1, 32)), F.OUT("responses", resp.reshape(-1, 32)), F.OUT("status", np.zeros(n, np.uint8))]
                return head + [t, inst, com, F.IN("challenges", chal.reshape(-1, 32)), F.IN("responses", resp.reshape(-1, 32))] + tail + [
                    F.OUT("results", np.zeros(n, np.uint8))]
            fp, fv = FOOTPRINT_FUNCTIONS[form]
            variant = "t%d" % threads if form == "batch" else ""
            out.append(F.Case(fp, form, n, variant, build))
            out.append(F.Case(fv, form, n, variant, functools.partial(build, prove=False)))
    return out

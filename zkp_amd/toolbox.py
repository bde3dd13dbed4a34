"""Python binding of the host toolbox (include/zkp_toolbox.h -> libzkp_toolbox.so), shaped like the
reference's API so tests read like the reference's tests:

    reference (Rust)                                   here
    -------------------------------------------------  ----------------------------------------------
    Transcript::new(b"..")                             Transcript(b"..")
    toolbox::prover::Prover::new(label, &mut t)        Prover(label, t, engine)
    prover.allocate_scalar / allocate_point / constrain / prove_compact / prove_batchable
    toolbox::verifier::Verifier                        Verifier(label, t, engine)
    toolbox::batch_verifier::BatchVerifier             BatchVerifier(label, n, transcripts, engine)
    define_proof! { name, "label", (secrets), (instance), (common) : constraints }
                                                       define_proof(name, label, secrets, instance, common, constraints)

All arithmetic happens in the C++ host library and, below it, in the HIP library; this file only
marshals buffers.  Points are 32-byte ristretto255 encodings, scalars 32-byte little-endian strings
(ints are accepted and reduced mod l for convenience).
"""
from __future__ import annotations

import ctypes
import weakref
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import cabi
from .engine import Engine, load_library

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzkp_toolbox.so")
TRANSCRIPT_BYTES = 208
L = 2**252 + 27742317777372353535851937790883648493

EXPORTS = tuple(cabi.signatures("zkp_toolbox.h"))
ZKP_JOB_SHARED_TRANSCRIPT = 1
ZKP_TB_PIPE_FULL = 3


class ProofError(Exception):
    """src/errors.rs"""


class VerificationFailure(ProofError):
    pass


class BatchSizeMismatch(ProofError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        load_library()          # libzkp_mi355x.so must exist: no CPU fallback
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        _lib = cabi.bind(cabi.bind(cabi.bind(ctypes.CDLL(LIB_PATH), "zkp_toolbox.h"), "zkp_or_toolbox.h"), "zkp_or_batch_toolbox.h")
    return _lib


def set_fused_min_batch(n: int) -> None:
    """Batches of >= n proofs run transcripts, scalars and MSMs on the device; smaller ones hash on the host threads."""
    lib().zkp_toolbox_set_fused_min_batch(n)


def set_host_max_terms(n: int) -> None:
    """Calls of at most n (scalar, point) terms run on the host backend even with a GPU context (0 = never); ctx = None always does."""
    lib().zkp_toolbox_set_host_max_terms(n)


def get_host_max_terms() -> int:
    return lib().zkp_toolbox_get_host_max_terms()


class HostEngine:
    """Stands where an Engine stands in the calls of this module and selects the host backend (ctx == NULL in the C ABI): no GPU needed."""
    _h = None

    def close(self):
        pass


def get_fused_min_batch() -> int:
    return lib().zkp_toolbox_get_fused_min_batch()


def pipe_shard_plan(n_items: int, n_contexts: int, unit: int = 1, fused_min_batch: Optional[int] = None):
    """The contiguous ranges zkp_pipe_prove_batch / zkp_pipe_batch_verify[_many] ... cut n_items proofs (batches of `unit` proofs) into, one per
    context: [(lo, hi)] for contexts 0 .. G - 1 (zkp_pipe_shard_plan; plain arithmetic, no GPU)."""
    lo = np.zeros(max(1, n_contexts), np.uint32)
    hi = np.zeros(max(1, n_contexts), np.uint32)
    g = lib().zkp_pipe_shard_plan(n_items, unit, n_contexts, get_fused_min_batch() if fused_min_batch is None else fused_min_batch, _p(lo), _p(hi))
    return [(int(lo[i]), int(hi[i])) for i in range(int(g))]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def scalar_bytes(x) -> bytes:
    if isinstance(x, (bytes, bytearray)):
        assert len(x) == 32
        return bytes(x)
    if isinstance(x, np.ndarray):
        return x.tobytes()
    return (int(x) % L).to_bytes(32, "little")


def _raise(rc: int, what: str):
    if rc == 1:
        raise VerificationFailure()
    if rc == 2:
        raise BatchSizeMismatch()
    if rc != 0:
        from .engine import ZkpError
        raise ZkpError(f"{what} failed with code {rc}: {load_library().zkp_last_error().decode()}")


# ---------------------------------------------------------------------------------------------------
class Transcript:
    """merlin::Transcript (plain 208-byte state; clone() is a copy)."""

    def __init__(self, label: bytes = b"", _state: Optional[np.ndarray] = None):
        if _state is not None:
            self.state = _state.copy()
        else:
            self.state = np.zeros(TRANSCRIPT_BYTES, np.uint8)
            lib().zkp_transcript_init(_p(self.state), label, len(label))

    def clone(self) -> "Transcript":
        return Transcript(_state=self.state)

    def append_message(self, label: bytes, message: bytes) -> None:
        rc = lib().zkp_transcript_append_message(_p(self.state), label, message, len(message))
        if rc != 0:
            raise ValueError("zkp_transcript_append_message: code %d (messages and labels are limited to 2^32 - 1 bytes, as in merlin)" % rc)

    def challenge_bytes(self, label: bytes, n: int) -> bytes:
        out = ctypes.create_string_buffer(n)
        rc = lib().zkp_transcript_challenge_bytes(_p(self.state), label, out, n)
        if rc != 0:
            raise ValueError("zkp_transcript_challenge_bytes: code %d" % rc)
        return out.raw


def _scalar_canonical(b: bytes) -> bool:
    return len(b) == 32 and int.from_bytes(b, "little") < L


def _wire_decode(kind: str, buf: bytes, allow_trailing: bool):
    """The C codec of include/zkp_toolbox.h (zkp_proof_*_decode): -> (challenge | commitments, responses)."""
    buf = bytes(buf)
    cap = len(buf) // 32 + 1
    a = np.zeros((cap, 32), np.uint8)
    r = np.zeros((cap, 32), np.uint8)
    na, nr, used = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0)
    if kind == "compact":
        rc = lib().zkp_proof_compact_decode(buf, len(buf), _p(a), _p(r), cap, ctypes.byref(nr), ctypes.byref(used))
    else:
        rc = lib().zkp_proof_batchable_decode(buf, len(buf), _p(a), cap, ctypes.byref(na), _p(r), cap, ctypes.byref(nr), ctypes.byref(used))
    if rc != 0:
        raise ValueError("malformed proof (truncated, or a scalar was not canonically encoded): code %d" % rc)
    if not allow_trailing and used.value != len(buf):
        raise ValueError("trailing bytes")
    return ([x.tobytes() for x in a[:na.value]] if kind != "compact" else a[0].tobytes()), [x.tobytes() for x in r[:nr.value]]


@dataclass
class CompactProof:            # src/proofs.rs:15-20
    challenge: bytes
    responses: List[bytes]

    # Wire format = what `bincode::serialize` (bincode 1.x top-level functions: fixed-width little-endian integers, u64
    # sequence lengths) produces for the serde-derived struct (proofs.rs:14): Scalar serialises as a 32-byte tuple (no
    # length), Vec<Scalar> as u64 length + elements.  The codec itself is C (include/zkp_toolbox.h, zkp_proof_*): this
    # class only marshals.  The reference's tests only round-trip it (tests/zkp.rs:53-54), so there are no golden bytes
    # to pin; dalek rejects non-canonical scalars on deserialisation, and so does the decoder.  allow_trailing = True is
    # bincode's own behaviour (its top-level deserialize ignores what follows the value); the default here is strict.
    def to_bytes(self) -> bytes:
        m = len(self.responses)
        out = ctypes.create_string_buffer(lib().zkp_proof_compact_size(m))
        resp = np.frombuffer(b"".join(self.responses), np.uint8) if m else np.zeros(0, np.uint8)
        rc = lib().zkp_proof_compact_encode(bytes(self.challenge), _p(resp), m, out, len(out))
        if rc != 0:
            raise ValueError("zkp_proof_compact_encode: code %d" % rc)
        return out.raw

    @classmethod
    def from_bytes(cls, buf: bytes, allow_trailing: bool = False) -> "CompactProof":
        c, r = _wire_decode("compact", buf, allow_trailing)
        return cls(c, r)


@dataclass
class BatchableProof:          # src/proofs.rs:27-32
    commitments: List[bytes]
    responses: List[bytes]

    def to_bytes(self) -> bytes:
        nc, m = len(self.commitments), len(self.responses)
        out = ctypes.create_string_buffer(lib().zkp_proof_batchable_size(nc, m))
        coms = np.frombuffer(b"".join(self.commitments), np.uint8) if nc else np.zeros(0, np.uint8)
        resp = np.frombuffer(b"".join(self.responses), np.uint8) if m else np.zeros(0, np.uint8)
        rc = lib().zkp_proof_batchable_encode(_p(coms), nc, _p(resp), m, out, len(out))
        if rc != 0:
            raise ValueError("zkp_proof_batchable_encode: code %d" % rc)
        return out.raw

    @classmethod
    def from_bytes(cls, buf: bytes, allow_trailing: bool = False) -> "BatchableProof":
        k, r = _wire_decode("batchable", buf, allow_trailing)
        return cls(k, r)      # CompressedRistretto deserialises from any 32 bytes; validity is checked at decompress


class Statement:
    """Owns a zkp_statement handle.  Variables are registered in allocation order."""

    def __init__(self, proof_label: bytes):
        self.proof_label = proof_label
        self._h = ctypes.c_void_p(lib().zkp_statement_new(proof_label))
        self.secrets: List[bytes] = []
        self.points: List[Tuple[bytes, bool]] = []
        self.constraints: List[Tuple[int, List[Tuple[int, int]]]] = []

    def __del__(self):
        try:
            if self._h:
                lib().zkp_statement_free(self._h)
                self._h = None
        except Exception:
            pass

    def add_secret(self, name: bytes) -> int:
        self.secrets.append(name)
        return lib().zkp_statement_add_secret(self._h, name)

    def add_point(self, name: bytes, common: bool) -> int:
        self.points.append((name, common))
        return lib().zkp_statement_add_point(self._h, name, int(common))

    def constrain(self, lhs: int, lc: Sequence[Tuple[int, int]]) -> None:
        sc = np.array([s for s, _ in lc], dtype=np.uint32)
        pt = np.array([p for _, p in lc], dtype=np.uint32)
        rc = lib().zkp_statement_constrain(self._h, lhs, len(lc), _p(sc), _p(pt))
        if rc != 0:
            raise ValueError("bad constraint")
        self.constraints.append((lhs, list(lc)))

    @property
    def m(self): return len(self.secrets)
    @property
    def ni(self): return sum(1 for _, c in self.points if not c)
    @property
    def ns(self): return sum(1 for _, c in self.points if c)
    @property
    def nc(self): return len(self.constraints)
    @property
    def terms(self): return sum(len(lc) for _, lc in self.constraints)


def _transcripts_array(transcripts: Sequence[Transcript]) -> np.ndarray:
    return np.stack([t.state for t in transcripts]) if transcripts else np.zeros((0, TRANSCRIPT_BYTES), np.uint8)


def _store_transcripts(transcripts: Sequence[Transcript], arr: np.ndarray) -> None:
    for t, row in zip(transcripts, arr):
        t.state[:] = row


# ---- batched entry points (numpy arrays in the layouts of include/zkp_toolbox.h) -------------------
def prove_batch(eng: Engine, st: Statement, transcripts: np.ndarray, secrets: np.ndarray, inst: np.ndarray,
                common: np.ndarray, entropy: Optional[np.ndarray] = None, threads: int = 0, out=None):
    """-> (challenges[N][32], responses[N][m][32], commitments[N][nc][32]); transcripts advanced in place.
    out = (challenges, responses, commitments) to fill (C-contiguous uint8 arrays of those shapes, e.g. from pinned_empty: the engine's copies
    out are then true DMA that leaves under the call's last kernels); default: fresh arrays."""
    n = len(transcripts)
    _check_batch_shapes(st, n, inst, common, None, secrets)
    if entropy is not None and tuple(np.shape(entropy)) != (n, 32):
        raise ValueError("entropy must have shape (%d, 32)" % n)
    if out is None:
        chal = np.zeros((n, 32), np.uint8)
        resp = np.zeros((n, st.m, 32), np.uint8)
        coms = np.zeros((n, st.nc, 32), np.uint8)
    else:
        chal, resp, coms = out
        for name, a, shape in (("challenges", chal, (n, 32)), ("responses", resp, (n, st.m, 32)), ("commitments", coms, (n, st.nc, 32))):
            if tuple(np.shape(a)) != shape or a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"]:
                raise ValueError("out: %s must be a C-contiguous uint8 array of shape %r" % (name, shape))
    rc = lib().zkp_prove_batch(eng._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(secrets)),
                               _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                               _p(None if entropy is None else np.ascontiguousarray(entropy)), threads, _p(chal), _p(resp), _p(coms))
    _raise(rc, "zkp_prove_batch")
    return chal, resp, coms


def verify_compact_batch(eng, st, transcripts, inst, common, challenges, responses, threads: int = 0) -> np.ndarray:
    n = len(transcripts)
    _check_batch_shapes(st, n, inst, common, None, responses)
    if tuple(np.shape(challenges)) != (n, 32):
        raise ValueError("challenges must have shape (%d, 32)" % n)
    res = np.ones(n, np.uint8)
    rc = lib().zkp_verify_compact_batch(eng._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(inst)),
                                        _p(np.ascontiguousarray(common)), _p(np.ascontiguousarray(challenges)),
                                        _p(np.ascontiguousarray(responses)), threads, _p(res))
    _raise(rc, "zkp_verify_compact_batch")
    return res


def verify_batchable_each(eng, st, transcripts, inst, common, commitments, responses, weights16=None, threads: int = 0) -> np.ndarray:
    n = len(transcripts)
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16, per_proof_weights=True)
    res = np.ones(n, np.uint8)
    rc = lib().zkp_verify_batchable_each(eng._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(inst)),
                                         _p(np.ascontiguousarray(common)), _p(np.ascontiguousarray(commitments)),
                                         _p(np.ascontiguousarray(responses)),
                                         _p(None if weights16 is None else np.ascontiguousarray(weights16)), threads, _p(res))
    _raise(rc, "zkp_verify_batchable_each")
    return res


def _check_batch_shapes(st, n, inst, common, commitments, responses, weights16=None, per_proof_weights=False) -> None:
    """The C side reads [ni][N][32], [ns][32], [N][nc][32], [N][m][32] and [nc][N][16] (or [N][nc][16]) straight from these
    buffers: anything else would be an out-of-bounds read, so it is refused here."""
    def want(name, a, shape):
        if a is not None and (tuple(np.shape(a)) != shape or np.asarray(a).dtype != np.uint8):
            raise ValueError("%s must be a uint8 array of shape %r, got %r" % (name, shape, tuple(np.shape(a))))
    want("inst", inst, (st.ni, n, 32))
    want("common", common, (st.ns, 32))
    want("commitments", commitments, (n, st.nc, 32))
    want("responses", responses, (n, st.m, 32))
    want("weights16", weights16, (n, st.nc, 16) if per_proof_weights else (st.nc, n, 16))


def batch_verify(eng, st, transcripts, inst, common, commitments, responses, weights16=None, threads: int = 0,
                 batch_size: Optional[int] = None) -> None:
    """Raises VerificationFailure / BatchSizeMismatch like BatchVerifier::verify_batchable."""
    n = len(commitments)
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
    rc = lib().zkp_batch_verify(eng._h, st._h, n if batch_size is None else batch_size, len(transcripts), _p(transcripts),
                                _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                _p(None if weights16 is None else np.ascontiguousarray(weights16)), threads)
    _raise(rc, "zkp_batch_verify")


def batch_verify_many(eng, st, n_batches: int, transcripts, inst, common, commitments, responses, weights16=None, threads: int = 0) -> np.ndarray:
    """zkp_batch_verify_many: n_batches independent BatchVerifier::verify_batchable runs over consecutive ranges of the
    len(commitments) proofs -> verdicts[n_batches] (0 = Ok, 1 = VerificationFailure)."""
    n = len(commitments)
    if n_batches <= 0 or n % n_batches:
        raise ValueError("the number of proofs must be a positive multiple of n_batches")
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
    verdicts = (ctypes.c_int * n_batches)(*([1] * n_batches))
    rc = lib().zkp_batch_verify_many(eng._h, st._h, n_batches, n // n_batches, len(transcripts),
                                     _p(transcripts), _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                     _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                     _p(None if weights16 is None else np.ascontiguousarray(weights16)), threads, verdicts)
    _raise(rc, "zkp_batch_verify_many")
    return np.array(list(verdicts), np.int32)


def batch_verify_locate(eng, st, transcripts, inst, common, commitments, responses, weights16=None, threads: int = 0):
    """zkp_batch_verify_locate: the batch check and, if it fails, which proofs fail -> (ok, results[N]): ok = the batch
    verified (results then all 0); otherwise results[j] = 1 for the proofs that fail on their own.  A failed batch whose
    per-proof pass finds nothing (the C contract allows it) is still ok = False: never read success from results alone."""
    n = len(commitments)
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
    res = np.ones(n, np.uint8)
    rc = lib().zkp_batch_verify_locate(eng._h, st._h, n, len(transcripts), _p(transcripts),
                                       _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                       _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                       _p(None if weights16 is None else np.ascontiguousarray(weights16)), threads, _p(res))
    if rc not in (0, 1):
        _raise(rc, "zkp_batch_verify_locate")
    return rc == 0, res


def batch_verify_coeffs(eng, st, transcripts, inst, common, commitments, responses, weights16, threads: int = 0):
    """batch_verify that also returns the coefficient vector built on the GPU; (ok: bool, coeffs [total][32])."""
    n = len(commitments)
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
    total = st.ns + (st.ni + st.nc) * n
    co = np.zeros((total, 32), np.uint8)
    rc = lib().zkp_batch_verify_coeffs(eng._h, st._h, n, len(transcripts), _p(transcripts),
                                       _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                       _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                       _p(np.ascontiguousarray(weights16)), threads, _p(co))
    if rc not in (0, 1):
        _raise(rc, "zkp_batch_verify_coeffs")
    return rc == 0, co


def batch_verify_build(st, transcripts, inst, common, commitments, responses, weights16, threads: int = 0):
    """Host-only half of batch_verify: the exact MSM operands (no GPU needed)."""
    n = len(commitments)
    _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
    total = st.ns + (st.ni + st.nc) * n
    ms = np.zeros((total, 32), np.uint8)
    mp = np.zeros((total, 32), np.uint8)
    rc = lib().zkp_batch_verify_build(st._h, n, len(transcripts), _p(transcripts),
                                      _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                      _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                      _p(np.ascontiguousarray(weights16)), threads, _p(ms), _p(mp))
    _raise(rc, "zkp_batch_verify_build")
    return ms, mp


# ---- hash to the group (RFC 9496 section 4.3.4) ------------------------------------------------------------------------
def from_uniform_bytes(eng, inp, threads: int = 0) -> np.ndarray:
    """RistrettoPoint::from_uniform_bytes of every 64-byte row: [n][64] -> canonical encodings [n][32].  eng = None (or a HostEngine)
    maps on the host threads; with an Engine, calls above get_host_max_terms() outputs map on the GPU."""
    inp = np.ascontiguousarray(inp, dtype=np.uint8).reshape(-1, 64) if len(inp) else np.zeros((0, 64), np.uint8)
    out = np.zeros((len(inp), 32), np.uint8)
    rc = lib().zkp_from_uniform_bytes_batch(None if eng is None else eng._h, len(inp), _p(inp), threads, _p(out))
    _raise(rc, "zkp_from_uniform_bytes_batch")
    return out


def hash_to_group(eng, transcripts, label: bytes = b"output", threads: int = 0) -> np.ndarray:
    """N x { challenge_bytes(label, 64) ; from_uniform_bytes } -- the `hash_to_group` of the reference's VRF example
    (tests/sig_and_vrf_example.rs:36-40) -- -> encodings [N][32].  transcripts: a list of Transcript objects or a [N][208] uint8
    array (C-contiguous); either is advanced in place exactly as merlin advances it."""
    objs = None
    if len(transcripts) and isinstance(transcripts[0], Transcript):
        objs, arr = transcripts, _transcripts_array(transcripts)
    else:
        arr = transcripts if len(transcripts) else np.zeros((0, TRANSCRIPT_BYTES), np.uint8)
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and arr.ndim == 2 and arr.shape[1] == TRANSCRIPT_BYTES and arr.flags["C_CONTIGUOUS"]):
            raise ValueError("transcripts must be Transcript objects or a C-contiguous uint8 array of shape [N][%d]" % TRANSCRIPT_BYTES)
    out = np.zeros((len(arr), 32), np.uint8)
    rc = lib().zkp_hash_to_group_batch(None if eng is None else eng._h, len(arr), _p(arr), label, threads, _p(out))
    _raise(rc, "zkp_hash_to_group_batch")
    if objs is not None:
        _store_transcripts(objs, arr)
    return out


def append_messages(ts_or_label, label: bytes, messages, threads: int = 0, eng=None) -> np.ndarray:
    """merlin append_message(label, messages[j]) for every transcript j.  ts_or_label: a [N][208] uint8 array (C-contiguous, advanced in
    place) or a bytes label (N fresh Transcript(label) states).  Returns the [N][208] states.  eng = None (or a HostEngine) appends on the
    host threads; with an Engine, batches above get_host_max_terms() transcripts whose messages average 128 bytes or more append on the GPU,
    one lane per transcript.  Same bytes either way."""
    from .engine import messages_csr
    return append_messages_csr(ts_or_label, label, *messages_csr(messages), threads=threads, eng=eng)


def append_messages_csr(ts_or_label, label: bytes, data, offsets, threads: int = 0, eng=None) -> np.ndarray:
    """append_messages over a CSR batch: message j = data[offsets[j]:offsets[j + 1]] (offsets: N + 1 entries, non-decreasing, uint64)"""
    from .engine import _csr_args
    data, offsets = _csr_args(data, offsets)
    n = len(offsets) - 1
    shared = isinstance(ts_or_label, (bytes, bytearray))
    if shared:
        ts = np.zeros((max(n, 1), TRANSCRIPT_BYTES), np.uint8)
        ts[0] = Transcript(bytes(ts_or_label)).state
        ts = ts[:n] if n else ts[:0]
    else:
        ts = ts_or_label
        if not (isinstance(ts, np.ndarray) and ts.dtype == np.uint8 and ts.shape == (n, TRANSCRIPT_BYTES) and ts.flags["C_CONTIGUOUS"]):
            raise ValueError("transcripts must be a C-contiguous uint8 array of shape [N][%d] with N = len(offsets) - 1" % TRANSCRIPT_BYTES)
    h = None if eng is None else eng._h
    if h is None:
        rc, what = lib().zkp_transcripts_append_message_batch(_p(ts), n, int(shared), bytes(label), _p(data), _p(offsets), threads), "zkp_transcripts_append_message_batch"
    else:
        rc, what = lib().zkp_transcripts_append_message_batch_ctx(h, _p(ts), n, int(shared), bytes(label), _p(data), _p(offsets), threads), "zkp_transcripts_append_message_batch_ctx"
    if rc != 0:
        raise ValueError("%s: code %d (messages and labels are limited to 2^32 - 1 bytes, as in merlin)" % (what, rc))
    return ts


def challenge_bytes(eng, transcripts, label: bytes, n: int, threads: int = 0) -> np.ndarray:
    """merlin challenge_bytes(label, n bytes) of every transcript -> [N][n] uint8; transcripts: a C-contiguous [N][208] uint8 array, advanced
    in place.  Routed as append_messages: eng = None (or a HostEngine) on the host threads, otherwise batches above get_host_max_terms()
    transcripts on the GPU."""
    ts = transcripts
    if not (isinstance(ts, np.ndarray) and ts.dtype == np.uint8 and ts.ndim == 2 and ts.shape[1] == TRANSCRIPT_BYTES and ts.flags["C_CONTIGUOUS"]):
        raise ValueError("transcripts must be a C-contiguous uint8 array of shape [N][%d]" % TRANSCRIPT_BYTES)
    if not 0 <= n <= 0xffffffff:
        raise ValueError("challenge_bytes: outputs are limited to 2^32 - 1 bytes, as in merlin")
    out = np.zeros((len(ts), n), np.uint8)
    rc = lib().zkp_transcripts_challenge_bytes_batch(None if eng is None else eng._h, _p(ts), len(ts), bytes(label), n, threads, _p(out))
    _raise(rc, "zkp_transcripts_challenge_bytes_batch")
    return out


# ---- the rest of TranscriptProtocol and the prover's TranscriptRng, batched (include/zkp_toolbox.h): eng = None is the host threads ----
RNG_SCALARS, RNG_BYTES = 0, 1        # ZKP_RNG_SCALARS, ZKP_RNG_BYTES


def _blob_array(ts, what: str) -> np.ndarray:
    if not (isinstance(ts, np.ndarray) and ts.dtype == np.uint8 and ts.ndim == 2 and ts.shape[1] == TRANSCRIPT_BYTES and ts.flags["C_CONTIGUOUS"]):
        raise ValueError("%s: transcripts must be a C-contiguous uint8 array of shape [N][%d]" % (what, TRANSCRIPT_BYTES))
    return ts


def _witness_rng(eng, transcripts, witnesses, mode: int, count: int, entropy, label: bytes, threads: int) -> np.ndarray:
    ts = _blob_array(transcripts, "witness_rng")
    n = len(ts)
    wit = np.ascontiguousarray(witnesses, np.uint8)
    if wit.ndim != 3 or len(wit) != n:
        raise ValueError("witness_rng: witnesses must be uint8 [N][m][wlen]")
    ent = None if entropy is None else np.ascontiguousarray(entropy, np.uint8)
    if ent is not None and ent.shape != (n, 32):
        raise ValueError("witness_rng: entropy must be uint8 [N][32] (or None: drawn from the operating system)")
    if not 0 <= count <= 0xffffffff:
        raise ValueError("witness_rng: count must fit 32 bits")
    out = np.zeros((n, count, 32) if mode == RNG_SCALARS else (n, count), np.uint8)
    rc = lib().zkp_transcripts_witness_rng_batch(None if eng is None else eng._h, _p(ts), n, bytes(label), wit.shape[1], wit.shape[2], _p(wit), _p(ent), mode,
                                                 count, threads, _p(out))
    _raise(rc, "zkp_transcripts_witness_rng_batch")
    return out


def witness_rng_scalars(eng, transcripts, witnesses, count: int, entropy=None, label: bytes = b"", threads: int = 0) -> np.ndarray:
    """The prover's synthetic nonces (reference src/toolbox/prover.rs:78-89) for every transcript: build_rng(), rekey_with_witness_bytes(label,
    witnesses[j][k]) for every k, finalize with entropy[j] (None: 32 bytes per transcript from the operating system), then count x
    Scalar::random -> canonical scalars uint8 [N][count][32].  transcripts: C-contiguous uint8 [N][208], read and never changed (build_rng
    clones); witnesses: uint8 [N][m][wlen].  eng = None (or a HostEngine) runs on the host threads; with an Engine, batches of at least
    get_witness_rng_min_batch() transcripts run on the GPU, one lane per transcript.  Same bytes either way."""
    return _witness_rng(eng, transcripts, witnesses, RNG_SCALARS, count, entropy, label, threads)


def witness_rng_bytes(eng, transcripts, witnesses, count: int, entropy=None, label: bytes = b"", threads: int = 0) -> np.ndarray:
    """witness_rng_scalars with one fill_bytes(count) in place of the scalars -> uint8 [N][count]"""
    return _witness_rng(eng, transcripts, witnesses, RNG_BYTES, count, entropy, label, threads)


def challenge_scalars(eng, transcripts, label: bytes, threads: int = 0) -> np.ndarray:
    """TranscriptProtocol::get_challenge(label) of every transcript: challenge_bytes(label, 64) reduced mod l -> canonical scalars uint8
    [N][32]; transcripts (C-contiguous uint8 [N][208]) advance in place.  Routed by get_challenge_scalars_min_batch()."""
    ts = _blob_array(transcripts, "challenge_scalars")
    out = np.zeros((len(ts), 32), np.uint8)
    rc = lib().zkp_transcripts_challenge_scalars_batch(None if eng is None else eng._h, _p(ts), len(ts), bytes(label), threads, _p(out))
    _raise(rc, "zkp_transcripts_challenge_scalars_batch")
    return out


def _append_points(eng, transcripts, kind: bytes, label: bytes, points, validate: bool, threads: int) -> np.ndarray:
    ts = _blob_array(transcripts, "append_points")
    pts = np.ascontiguousarray(points, np.uint8)
    if pts.shape != (len(ts), 32):
        raise ValueError("append_points: points must be uint8 [N][32]")
    status = np.zeros(len(ts), np.uint8)
    rc = lib().zkp_transcripts_append_points_batch(None if eng is None else eng._h, _p(ts), len(ts), kind, bytes(label), _p(pts), int(bool(validate)), threads,
                                                   _p(status))
    _raise(rc, "zkp_transcripts_append_points_batch")
    return status


def append_point_vars(eng, transcripts, label: bytes, points, validate: bool = False, threads: int = 0) -> np.ndarray:
    """TranscriptProtocol::append_point_var(label, points[j]) on every transcript (C-contiguous uint8 [N][208], advanced in place); validate:
    validate_and_append_point_var, which refuses the identity's encoding.  -> status uint8 [N]: 1 = refused, that transcript is unchanged.
    Routed by get_append_points_min_batch()."""
    return _append_points(eng, transcripts, b"ptvar", label, points, validate, threads)


def append_blinding_commitments(eng, transcripts, label: bytes, points, validate: bool = False, threads: int = 0) -> np.ndarray:
    """TranscriptProtocol::append_blinding_commitment / validate_and_append_blinding_commitment, as append_point_vars"""
    return _append_points(eng, transcripts, b"blindcom", label, points, validate, threads)


def domain_sep(ts, label: bytes, threads: int = 0, eng=None) -> np.ndarray:
    """TranscriptProtocol::domain_sep(label) on every transcript of ts (uint8 [N][208], advanced in place)"""
    append_messages(ts, b"dom-sep", [b"schnorrzkp/1.0/ristretto255"] * len(ts), threads=threads, eng=eng)
    return append_messages(ts, b"dom-sep", [bytes(label)] * len(ts), threads=threads, eng=eng)


def append_scalar_vars(ts, label: bytes, threads: int = 0, eng=None) -> np.ndarray:
    """TranscriptProtocol::append_scalar_var(label) on every transcript of ts (uint8 [N][208], advanced in place)"""
    return append_messages(ts, b"scvar", [bytes(label)] * len(ts), threads=threads, eng=eng)


def set_witness_rng_min_batch(n: int) -> None:
    """witness_rng_* calls on an engine with at least n transcripts run on the device (0: always; 2**32 - 1: never)"""
    lib().zkp_toolbox_set_witness_rng_min_batch(n)


def get_witness_rng_min_batch() -> int:
    return int(lib().zkp_toolbox_get_witness_rng_min_batch())


def set_challenge_scalars_min_batch(n: int) -> None:
    """challenge_scalars calls on an engine with at least n transcripts run on the device (0: always; 2**32 - 1: never)"""
    lib().zkp_toolbox_set_challenge_scalars_min_batch(n)


def get_challenge_scalars_min_batch() -> int:
    return int(lib().zkp_toolbox_get_challenge_scalars_min_batch())


def set_append_points_min_batch(n: int) -> None:
    """append_point_vars / append_blinding_commitments calls on an engine with at least n transcripts run on the device (0: always; 2**32 - 1: never)"""
    lib().zkp_toolbox_set_append_points_min_batch(n)


def get_append_points_min_batch() -> int:
    return int(lib().zkp_toolbox_get_append_points_min_batch())


# ---- batched 1-of-k OR-proofs (include/zkp_or_toolbox.h) --------------------------------------------
def _or_shapes(st, transcripts, inst, common, what: str):
    ts = _blob_array(transcripts, what)
    n = len(ts)
    inst = np.ascontiguousarray(inst, np.uint8)
    if inst.ndim != 4 or inst.shape[1:] != (st.ni, n, 32):
        raise ValueError("%s: inst must be uint8 [k][%d][%d][32]" % (what, st.ni, n))
    com = np.ascontiguousarray(common, np.uint8)
    if com.size != 32 * st.ns:
        raise ValueError("%s: common must be uint8 [%d][32]" % (what, st.ns))
    return ts, n, len(inst), inst, com


def or_prove(eng, st: Statement, transcripts, secrets, real, inst, common, entropy=None, threads: int = 0):
    """N disjunctions "I know a witness of ONE of these k instances of st" (Cramer-Damgard-Schoenmakers over the reference's prover steps;
    the protocol is stated in include/zkp_or_mi355x.h).  inst: uint8 [k][ni][N][32], branch b = st over inst[b] and the shared common points,
    k is taken from it; secrets [N][m][32]; real [N] = the branch each witness satisfies; entropy [N][32] or None (drawn from the operating
    system).  transcripts (C-contiguous uint8 [N][208], any mix of positions) advance in place.
    -> (challenges [N][k][32], responses [N][k][m][32], status [N]: 1 = a point of that proof did not decode, its rows are zeros).
    No branch, address or call sequence depends on real.  eng = None runs the host backend; with an Engine, batches of at least
    get_or_min_batch() proofs run on the GPU.  Same bytes either way."""
    ts, n, k, inst, com = _or_shapes(st, transcripts, inst, common, "or_prove")
    sec = np.ascontiguousarray(secrets, np.uint8)
    rl = np.ascontiguousarray(real, np.uint8)
    if sec.size != 32 * n * st.m or rl.shape != (n,):
        raise ValueError("or_prove: secrets must be uint8 [N][m][32] and real uint8 [N]")
    ent = None if entropy is None else np.ascontiguousarray(entropy, np.uint8)
    if ent is not None and ent.shape != (n, 32):
        raise ValueError("or_prove: entropy must be uint8 [N][32] (or None)")
    chal, resp, status = np.zeros((n, k, 32), np.uint8), np.zeros((n, k, st.m, 32), np.uint8), np.zeros(n, np.uint8)
    rc = lib().zkp_or_prove_batch(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(sec), _p(rl), _p(inst), _p(com), _p(ent), threads, _p(chal), _p(resp),
                                  _p(status))
    _raise(rc, "zkp_or_prove_batch")
    return chal, resp, status


def or_verify(eng, st: Statement, transcripts, inst, common, challenges, responses, threads: int = 0) -> np.ndarray:
    """The verifier of or_prove's proofs -> results uint8 [N]: 0 = accepted, 1 = rejected.  transcripts advance in place (an accepted
    proof's ends where the prover's ended)."""
    ts, n, k, inst, com = _or_shapes(st, transcripts, inst, common, "or_verify")
    chal = np.ascontiguousarray(challenges, np.uint8)
    resp = np.ascontiguousarray(responses, np.uint8)
    if chal.shape != (n, k, 32) or resp.size != 32 * n * k * st.m:
        raise ValueError("or_verify: challenges must be uint8 [N][k][32] and responses uint8 [N][k][m][32]")
    res = np.ones(n, np.uint8)
    rc = lib().zkp_or_verify_batch(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(inst), _p(com), _p(chal), _p(resp), threads, _p(res))
    _raise(rc, "zkp_or_verify_batch")
    return res


def set_or_min_batch(n: int) -> None:
    """or_prove / or_verify calls on an engine with at least n proofs run on the device (0: always; 2**32 - 1: never)"""
    lib().zkp_toolbox_set_or_min_batch(n)


def get_or_min_batch() -> int:
    return int(lib().zkp_toolbox_get_or_min_batch())


# ---- batchable 1-of-k OR-proofs (include/zkp_or_batch_toolbox.h) -------------------------------------
def or_prove_batchable(eng, st: Statement, transcripts, secrets, real, inst, common, entropy=None, threads: int = 0):
    """or_prove plus the commitments the prover appended -> (commitments [N][k][nc][32], challenges [N][k][32], responses [N][k][m][32],
    status [N]).  Challenges, responses, status and transcripts are or_prove's bytes; the commitments of a proof with status 1 are
    unspecified."""
    ts, n, k, inst, com = _or_shapes(st, transcripts, inst, common, "or_prove_batchable")
    sec = np.ascontiguousarray(secrets, np.uint8)
    rl = np.ascontiguousarray(real, np.uint8)
    if sec.size != 32 * n * st.m or rl.shape != (n,):
        raise ValueError("or_prove_batchable: secrets must be uint8 [N][m][32] and real uint8 [N]")
    ent = None if entropy is None else np.ascontiguousarray(entropy, np.uint8)
    if ent is not None and ent.shape != (n, 32):
        raise ValueError("or_prove_batchable: entropy must be uint8 [N][32] (or None)")
    coms, chal = np.zeros((n, k, st.nc, 32), np.uint8), np.zeros((n, k, 32), np.uint8)
    resp, status = np.zeros((n, k, st.m, 32), np.uint8), np.zeros(n, np.uint8)
    rc = lib().zkp_or_prove_batchable_batch(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(sec), _p(rl), _p(inst), _p(com), _p(ent), threads, _p(coms),
                                            _p(chal), _p(resp), _p(status))
    _raise(rc, "zkp_or_prove_batchable_batch")
    return coms, chal, resp, status


def _or_batchable_shapes(st, transcripts, inst, common, commitments, challenges, responses, weights16, what: str):
    ts, n, k, inst, com = _or_shapes(st, transcripts, inst, common, what)
    coms = np.ascontiguousarray(commitments, np.uint8)
    chal = np.ascontiguousarray(challenges, np.uint8)
    resp = np.ascontiguousarray(responses, np.uint8)
    if coms.shape != (n, k, st.nc, 32) or chal.shape != (n, k, 32) or resp.size != 32 * n * k * st.m:
        raise ValueError("%s: commitments must be uint8 [N][k][nc][32], challenges [N][k][32] and responses [N][k][m][32]" % what)
    w = None if weights16 is None else np.ascontiguousarray(weights16, np.uint8)
    if w is not None and w.shape != (n, k, st.nc, 16):
        raise ValueError("%s: weights16 must be uint8 [N][k][nc][16] (or None)" % what)
    return ts, n, k, inst, com, coms, chal, resp, w


def or_verify_batchable(eng, st: Statement, transcripts, inst, common, commitments, challenges, responses, threads: int = 0) -> np.ndarray:
    """The exact per-proof verifier of or_prove_batchable's proofs -> results uint8 [N]: 0 = accepted, 1 = rejected.  transcripts advance
    in place (an accepted proof's ends where the prover's ended)."""
    ts, n, k, inst, com, coms, chal, resp, _ = _or_batchable_shapes(st, transcripts, inst, common, commitments, challenges, responses, None,
                                                                    "or_verify_batchable")
    res = np.ones(n, np.uint8)
    rc = lib().zkp_or_verify_batchable_batch(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(inst), _p(com), _p(coms), _p(chal), _p(resp), threads,
                                             _p(res))
    _raise(rc, "zkp_or_verify_batchable_batch")
    return res


def or_batch_verify(eng, st: Statement, transcripts, inst, common, commitments, challenges, responses, weights16=None, threads: int = 0) -> bool:
    """One verdict for N batchable proofs: True = every proof verifies.  One multiscalar sum of ns + N k (ni + nc) operands under the
    weights r_jbc (weights16 uint8 [N][k][nc][16], None: drawn from the operating system); a wrong proof passes with probability 2^-128.
    eng = None, or fewer than get_or_batch_min_batch() proofs, runs the host backend: the same verdict."""
    ts, n, k, inst, com, coms, chal, resp, w = _or_batchable_shapes(st, transcripts, inst, common, commitments, challenges, responses, weights16,
                                                                    "or_batch_verify")
    rc = lib().zkp_or_batch_verify_batch(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(inst), _p(com), _p(coms), _p(chal), _p(resp), _p(w), threads)
    if rc not in (0, 1):
        _raise(rc, "zkp_or_batch_verify_batch")
    return rc == 0


def or_batch_verify_locate(eng, st: Statement, transcripts, inst, common, commitments, challenges, responses, weights16=None, threads: int = 0):
    """The batch check and, only if it fails, which proofs fail -> (ok, results [N]): ok = the batch verified (results then all 0);
    otherwise results[j] = 1 for the proofs or_verify_batchable rejects.  Never read success from results alone."""
    ts, n, k, inst, com, coms, chal, resp, w = _or_batchable_shapes(st, transcripts, inst, common, commitments, challenges, responses, weights16,
                                                                    "or_batch_verify_locate")
    res = np.ones(n, np.uint8)
    rc = lib().zkp_or_batch_verify_locate(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(inst), _p(com), _p(coms), _p(chal), _p(resp), _p(w), threads,
                                          _p(res))
    if rc not in (0, 1):
        _raise(rc, "zkp_or_batch_verify_locate")
    return rc == 0, res


def or_batch_verify_coeffs(eng, st: Statement, transcripts, inst, common, commitments, challenges, responses, weights16, threads: int = 0):
    """or_batch_verify that also returns the coefficient vector -> (ok, coeffs [ns + N k (ni + nc)][32]) over the operands
    [common | inst[b][v][j] | commitments [N][k][nc]]"""
    ts, n, k, inst, com, coms, chal, resp, w = _or_batchable_shapes(st, transcripts, inst, common, commitments, challenges, responses, weights16,
                                                                    "or_batch_verify_coeffs")
    co = np.zeros((st.ns + n * k * (st.ni + st.nc), 32), np.uint8)
    rc = lib().zkp_or_batch_verify_coeffs(None if eng is None else eng._h, st._h, k, n, _p(ts), _p(inst), _p(com), _p(coms), _p(chal), _p(resp), _p(w), threads,
                                          _p(co))
    if rc not in (0, 1):
        _raise(rc, "zkp_or_batch_verify_coeffs")
    return rc == 0, co


def set_or_batch_min_batch(n: int) -> None:
    """or_batch_verify (and _locate's and _coeffs' batch check) on an engine with at least n proofs runs on the device (0: always;
    2**32 - 1: never)"""
    lib().zkp_toolbox_set_or_batch_min_batch(n)


def get_or_batch_min_batch() -> int:
    return int(lib().zkp_toolbox_get_or_batch_min_batch())


def hash_from_bytes_sha512(eng, messages, threads: int = 0) -> np.ndarray:
    """RistrettoPoint::hash_from_bytes::<Sha512> (reference tests/zkp.rs:35) of every message (a list of byte strings) -> encodings
    [n][32].  eng = None (or a HostEngine) hashes and maps on the host threads; with an Engine, calls above get_host_max_terms()
    messages run both on the GPU."""
    from .engine import messages_csr
    return hash_from_bytes_sha512_csr(eng, *messages_csr(messages), threads=threads)


def hash_from_bytes_sha512_csr(eng, data, offsets, threads: int = 0) -> np.ndarray:
    """hash_from_bytes_sha512 of a CSR batch already held in numpy buffers: message i = data[offsets[i]:offsets[i + 1]] (offsets: n + 1
    entries, non-decreasing, uint64)."""
    from .engine import _csr_args
    data, offsets = _csr_args(data, offsets)
    n = len(offsets) - 1
    out = np.zeros((n, 32), np.uint8)
    rc = lib().zkp_hash_from_bytes_sha512_batch(None if eng is None else eng._h, n, _p(data), _p(offsets), threads, _p(out))
    _raise(rc, "zkp_hash_from_bytes_sha512_batch")
    return out


# ---- scalars mod l, batched (include/zkp_toolbox.h): canonical scalars [n][32] out; eng = None is the host backend ------------------------
def scalar_invert(eng, s, threads: int = 0) -> np.ndarray:
    """Scalar::invert (reference tests/zkp.rs:35) of every row of s [n][32] (any 32 bytes, read mod l; 0 -> 0)"""
    from .engine import _u8
    s = _u8(s, 32)
    out = np.zeros((len(s), 32), np.uint8)
    _raise(lib().zkp_scalar_invert_batch(None if eng is None else eng._h, len(s), _p(s), threads, _p(out)), "zkp_scalar_invert_batch")
    return out


def scalar_from_wide(eng, wide, threads: int = 0) -> np.ndarray:
    """Scalar::from_bytes_mod_order_wide of every row of wide [n][64]"""
    from .engine import _u8
    wide = _u8(wide, 64)
    out = np.zeros((len(wide), 32), np.uint8)
    _raise(lib().zkp_scalar_from_wide_batch(None if eng is None else eng._h, len(wide), _p(wide), threads, _p(out)), "zkp_scalar_from_wide_batch")
    return out


def scalar_muladd(eng, a, b, c=None, threads: int = 0) -> np.ndarray:
    """a * b + c mod l row by row (prover.rs:108 for a batch).  An operand of shape (32,) or (1, 32) is one scalar for every row; c = None: + 0."""
    from .engine import scalar_operands
    n, (a, sa), (b, sb), (c, sc) = scalar_operands(a, b, c)
    out = np.zeros((n, 32), np.uint8)
    _raise(lib().zkp_scalar_muladd_batch(None if eng is None else eng._h, n, _p(a), sa, _p(b), sb, _p(c), sc, threads, _p(out)), "zkp_scalar_muladd_batch")
    return out


def scalar_reduce(eng, op: int, off, a, aidx=None, b=None, bidx=None, threads: int = 0) -> np.ndarray:
    """zkp_scalar_reduce_batch: out[i] = the fold of the terms [off[i], off[i + 1]) -> [n_out][32] canonical scalars.  eng = None, or fewer than
    get_scalar_reduce_min_terms(op) terms, runs on the host threads, which share the TERM axis; anything else is Engine.scalar_reduce.  Same bytes."""
    from .engine import reduce_operands
    off, a, aidx, b, bidx = reduce_operands(op, off, a, aidx, b, bidx)
    n_out = len(off) - 1
    out = np.zeros((n_out, 32), np.uint8)
    _raise(lib().zkp_scalar_reduce_batch(None if eng is None else eng._h, op, n_out, _p(off), _p(a) if len(a) else None, len(a), _p(aidx),
                                         None if b is None or not len(b) else _p(b), 0 if b is None else len(b), _p(bidx), threads, _p(out)),
           "zkp_scalar_reduce_batch")
    return out


def scalar_sum(eng, off, a, aidx=None, threads: int = 0) -> np.ndarray:
    """`iter().sum()` per segment: out[i] = sum over t in [off[i], off[i + 1]) of a[aidx[t]] (aidx = None: a[t]); an empty segment is 0"""
    return scalar_reduce(eng, 0, off, a, aidx, threads=threads)


def scalar_product(eng, off, a, aidx=None, threads: int = 0) -> np.ndarray:
    """`iter().product()` per segment: out[i] = prod over t in [off[i], off[i + 1]) of a[aidx[t]] (aidx = None: a[t]); an empty segment is 1"""
    return scalar_reduce(eng, 1, off, a, aidx, threads=threads)


def scalar_dot(eng, off, a, b, aidx=None, bidx=None, threads: int = 0) -> np.ndarray:
    """inner products per segment: out[i] = sum over t in [off[i], off[i + 1]) of a[aidx[t]] * b[bidx[t]] (an index list None: row t); empty: 0"""
    return scalar_reduce(eng, 2, off, a, aidx, b, bidx, threads=threads)


def set_scalar_reduce_min_terms(op: int, n: int) -> None:
    """scalar_reduce jobs of op on an engine with at least n terms run on the device (0: always; 2**64 - 1: never)"""
    lib().zkp_toolbox_set_scalar_reduce_min_terms(op, n)


def get_scalar_reduce_min_terms(op: int) -> int:
    return int(lib().zkp_toolbox_get_scalar_reduce_min_terms(op))


def scalar_scan(eng, op: int, off, a, aidx=None, exclusive: bool = False, threads: int = 0) -> np.ndarray:
    """zkp_scalar_scan_batch: out[t] = the fold of the terms of t's segment up to t (exclusive: before t) -> [off[-1]][32] canonical scalars.  eng = None,
    or fewer than get_scalar_scan_min_terms(op) terms, runs on the host threads, which share the TERM axis; anything else is Engine.scalar_scan."""
    from .engine import reduce_operands
    off, a, aidx, _, _ = reduce_operands(0, off, a, aidx)
    out = np.zeros((int(off[-1]), 32), np.uint8)
    _raise(lib().zkp_scalar_scan_batch(None if eng is None else eng._h, op, int(bool(exclusive)), len(off) - 1, _p(off), _p(a) if len(a) else None, len(a),
                                       _p(aidx), threads, _p(out)), "zkp_scalar_scan_batch")
    return out


def scalar_cumsum(eng, off, a, aidx=None, exclusive: bool = False, threads: int = 0) -> np.ndarray:
    """running sums per segment: out[t] = sum of a[aidx[t']] over the terms t' <= t of t's segment (exclusive: t' < t; 0 at a segment's first term)"""
    return scalar_scan(eng, 0, off, a, aidx, exclusive, threads)


def scalar_cumprod(eng, off, a, aidx=None, exclusive: bool = False, threads: int = 0) -> np.ndarray:
    """running products per segment: out[t] = prod of a[aidx[t']] over the terms t' <= t of t's segment (exclusive: t' < t; 1 at a segment's first term)"""
    return scalar_scan(eng, 1, off, a, aidx, exclusive, threads)


def scalar_powers(eng, x, t: int, threads: int = 0) -> np.ndarray:
    """x [n][32] -> [n][t][32]: row j holds x[j]^0 .. x[j]^(t-1), an exclusive product scan over t references to row j"""
    from .engine import _u8
    x = _u8(x, 32)
    n = len(x)
    off = np.arange(n + 1, dtype=np.uint64) * t
    if int(off[-1]) > 0x7fffffff:
        raise ValueError("more than 2**31 - 1 powers")
    aidx = np.repeat(np.arange(n, dtype=np.uint32), t)
    return scalar_cumprod(eng, off.astype(np.uint32), x, aidx, True, threads).reshape(n, t, 32)


def set_scalar_scan_min_terms(op: int, n: int) -> None:
    """scalar_scan jobs of op on an engine with at least n terms run on the device (0: always; 2**64 - 1: never)"""
    lib().zkp_toolbox_set_scalar_scan_min_terms(op, n)


def get_scalar_scan_min_terms(op: int) -> int:
    return int(lib().zkp_toolbox_get_scalar_scan_min_terms(op))


def scalar_hash_from_bytes_sha512(eng, messages, threads: int = 0) -> np.ndarray:
    """Scalar::hash_from_bytes::<Sha512> of every message (a list of byte strings)"""
    from .engine import messages_csr
    return scalar_hash_from_bytes_sha512_csr(eng, *messages_csr(messages), threads=threads)


def scalar_hash_from_bytes_sha512_csr(eng, data, offsets, threads: int = 0) -> np.ndarray:
    """the same for a CSR batch held in numpy buffers: message i = data[offsets[i]:offsets[i + 1]]"""
    from .engine import _csr_args
    data, offsets = _csr_args(data, offsets)
    n = len(offsets) - 1
    out = np.zeros((n, 32), np.uint8)
    rc = lib().zkp_scalar_hash_from_bytes_sha512_batch(None if eng is None else eng._h, n, _p(data), _p(offsets), threads, _p(out))
    _raise(rc, "zkp_scalar_hash_from_bytes_sha512_batch")
    return out


def scalar_random(eng, n: int, key: Optional[bytes] = None, nonce: int = 0, threads: int = 0) -> np.ndarray:
    """n x Scalar::random (tests/sig_and_vrf_example.rs:49): row i = from_bytes_mod_order_wide(ChaCha20 block i of (key, nonce)); key = None
    takes 32 bytes from the operating system.  With an Engine and n above get_host_max_terms() the stream is drawn on the GPU."""
    k = None if key is None else np.frombuffer(bytes(key), np.uint8).copy()
    if k is not None and k.size != 32:
        raise ValueError("key must be 32 bytes")
    out = np.zeros((n, 32), np.uint8)
    _raise(lib().zkp_scalar_random_batch(None if eng is None else eng._h, n, _p(k), nonce, threads, _p(out)), "zkp_scalar_random_batch")
    return out


# ---- Scalar * basepoint, Scalar * point, multiscalar products (include/zkp_toolbox.h): encodings [n][32] out; eng = None is the host backend ----
def basepoint_mul(eng, scalars, threads: int = 0) -> np.ndarray:
    """scalars[i] * B for every row of scalars [n][32] (any 32 bytes, read mod l): `&sk * &RISTRETTO_BASEPOINT_TABLE` and compress()
    (PublicKey::from(&SecretKey), reference tests/sig_and_vrf_example.rs:58) for a batch; constant time"""
    from .engine import _u8
    s = _u8(scalars, 32)
    out = np.zeros((len(s), 32), np.uint8)
    _raise(lib().zkp_basepoint_mul_batch(None if eng is None else eng._h, len(s), _p(s), threads, _p(out)), "zkp_basepoint_mul_batch")
    return out


def point_mul(eng, scalars, points, flags: int = 1, threads: int = 0):
    """scalars[i] * decode(points[i]) row by row (`&H * &x`, tests/sig_and_vrf_example.rs:112) -> (encodings [n][32], status [n]); status 1 and a
    zero row where the point does not decode.  An operand of shape (32,) or (1, 32) is shared by every row.  flags = ZKP_CT (default) or
    ZKP_VARTIME."""
    from .engine import mul_operands
    n, (s, ss), (p, ps) = mul_operands(scalars, points)
    out = np.zeros((n, 32), np.uint8)
    status = np.zeros(n, np.uint8)
    _raise(lib().zkp_point_mul_batch(None if eng is None else eng._h, n, _p(s), ss, _p(p), ps, flags, threads, _p(out), _p(status)), "zkp_point_mul_batch")
    return out, status


def multiscalar_mul(eng, off, scalars, pidx, points, flags: int = 0, threads: int = 0):
    """Engine.msm_many behind the toolbox's routing (eng = None, or at most get_host_max_terms() terms: the host backend):
    out[i] = encode(sum over t in [off[i], off[i + 1]) of scalars[t] * decode(points[pidx[t]])) -> (out [n_msm][32], status [n_msm])"""
    from .engine import _u8
    off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
    pidx = np.ascontiguousarray(pidx, dtype=np.uint32).reshape(-1)
    if len(off) < 1:
        raise ValueError("off must hold n_msm + 1 entries")
    n_msm, n_terms = len(off) - 1, int(off[-1])
    scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
    points = _u8(points, 32)
    if len(scalars) != n_terms or len(pidx) != n_terms:
        raise ValueError("scalars / pidx length must equal off[-1]")
    out = np.zeros((n_msm, 32), np.uint8)
    status = np.zeros(n_msm, np.uint8)
    _raise(lib().zkp_multiscalar_mul_batch(None if eng is None else eng._h, n_msm, _p(off), _p(scalars), _p(pidx), _p(points), len(points), flags, threads,
                                           _p(out), _p(status)), "zkp_multiscalar_mul_batch")
    return out, status


def multiscalar_sum(eng, off, scalars, points, pidx=None, flags: int = 0, threads: int = 0):
    """multiscalar_mul's results for segments of ANY length -> (out [n_msm][32], status [n_msm]).  pidx = None: term t uses point t.  eng = None
    (or at most get_host_max_terms() terms) runs on the host threads, which share the TERM axis, so one long segment is everybody's work; with an
    Engine a job whose longest segment is below get_msm_fold_min_segment() is Engine.msm_many, anything else Engine.msm_segments.  Same bytes on
    every route."""
    from .engine import _u8, sum_operands
    off, pidx, _, points = sum_operands(off, points, pidx, None)
    n_msm, n_terms = len(off) - 1, int(off[-1])
    scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
    if len(scalars) != n_terms:
        raise ValueError("scalars length must equal off[-1]")
    out = np.zeros((n_msm, 32), np.uint8)
    status = np.zeros(n_msm, np.uint8)
    _raise(lib().zkp_multiscalar_sum_batch(None if eng is None else eng._h, n_msm, _p(off), _p(scalars), _p(pidx), _p(points), len(points), flags, threads,
                                           _p(out), _p(status)), "zkp_multiscalar_sum_batch")
    return out, status


def set_msm_fold_min_segment(n: int) -> None:
    """multiscalar_sum jobs on an engine whose longest segment has at least n terms fold the term axis (zkp_msm_segments); shorter ones are zkp_msm_many"""
    lib().zkp_toolbox_set_msm_fold_min_segment(n)


def get_msm_fold_min_segment() -> int:
    return int(lib().zkp_toolbox_get_msm_fold_min_segment())


def optional_multiscalar_mul(eng, off, scalars, points, pidx=None, threads: int = 0):
    """dalek's RistrettoPoint::optional_multiscalar_mul for a batch of segments, VARIABLE TIME (public scalars only): multiscalar_sum's results with
    ZKP_VARTIME -> (out [n_seg][32], status [n_seg]).  pidx = None: a point per term.  eng = None (or at most get_host_max_terms() terms) runs on the
    host threads; with an Engine a job whose longest segment is below get_msm_bucket_min_segment() takes multiscalar_sum's route, anything else
    Engine.msm_optional_many (the bucket method).  Same bytes on every route."""
    from .engine import _u8, sum_operands
    off, pidx, _, points = sum_operands(off, points, pidx, None)
    n_seg, n_terms = len(off) - 1, int(off[-1])
    scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
    if len(scalars) != n_terms:
        raise ValueError("scalars length must equal off[-1]")
    out = np.zeros((n_seg, 32), np.uint8)
    status = np.zeros(n_seg, np.uint8)
    _raise(lib().zkp_multiscalar_optional_batch(None if eng is None else eng._h, n_seg, _p(off), _p(scalars), _p(pidx), _p(points), len(points), threads,
                                                _p(out), _p(status)), "zkp_multiscalar_optional_batch")
    return out, status


def set_msm_bucket_min_segment(n: int) -> None:
    """optional_multiscalar_mul jobs on an engine whose longest segment has at least n terms take the bucket method (zkp_msm_optional_many); shorter
    ones go where multiscalar_sum sends them.  0xffffffff: never"""
    lib().zkp_toolbox_set_msm_bucket_min_segment(n)


def get_msm_bucket_min_segment() -> int:
    return int(lib().zkp_toolbox_get_msm_bucket_min_segment())


# ---- RistrettoPoint sums (include/zkp_toolbox.h): `P + Q`, `P - Q`, `-P`, `iter().sum()`, each with its compress(); eng = None is the host backend ----
def _point_pairs(eng, a, b, op: int, threads: int):
    from .engine import mul_operands
    n, (a, sa), (b, sb) = mul_operands(a, b)
    out = np.zeros((n, 32), np.uint8)
    status = np.zeros(n, np.uint8)
    _raise(lib().zkp_point_add_batch(None if eng is None else eng._h, n, _p(a), sa, _p(b), sb, op, threads, _p(out), _p(status)), "zkp_point_add_batch")
    return out, status


def point_add(eng, a, b, threads: int = 0):
    """decode(a[i]) + decode(b[i]) row by row -> (encodings [n][32], status [n]); status 1 and a zero row where an operand does not decode.  An
    operand of shape (32,) or (1, 32) is shared by every row."""
    return _point_pairs(eng, a, b, 0, threads)


def point_sub(eng, a, b, threads: int = 0):
    """decode(a[i]) - decode(b[i]) row by row; operands and results as point_add"""
    return _point_pairs(eng, a, b, 1, threads)


def point_neg(eng, a, threads: int = 0):
    """-decode(a[i]) for every row of a [n][32] (or one row of shape (32,)): the identity minus a"""
    return _point_pairs(eng, np.zeros(32, np.uint8), a, 1, threads)


def point_sum(eng, off, points, pidx=None, neg=None, threads: int = 0):
    """out[i] = encode(sum over t in [off[i], off[i + 1]) of +- decode(points[pidx[t]])) -> (out [n_sums][32], status [n_sums]): `iter().sum()` for a
    batch of ranges.  pidx = None: term t is point t.  neg = None: every term is added; else neg[t] != 0 subtracts term t.  An empty range is the
    identity (zero bytes, status 0); status 1 and a zero row where a referenced point does not decode."""
    from .engine import sum_operands
    off, pidx, neg, points = sum_operands(off, points, pidx, neg)
    n_sums = len(off) - 1
    out = np.zeros((n_sums, 32), np.uint8)
    status = np.zeros(n_sums, np.uint8)
    _raise(lib().zkp_point_sum_batch(None if eng is None else eng._h, n_sums, _p(off), _p(pidx), _p(neg), _p(points), len(points), threads, _p(out),
                                     _p(status)), "zkp_point_sum_batch")
    return out, status


def point_cumsum(eng, off, points, pidx=None, neg=None, exclusive: bool = False, threads: int = 0):
    """running sums of points per segment: out[t] = encode(sum of +- decode(points[pidx[t']]) over the terms t' <= t of t's segment) (exclusive:
    t' < t; the identity at a segment's first term) -> (out [off[-1]][32], status [off[-1]]).  pidx and neg as in point_sum.  status 1 and a zero row
    where a point the row depends on does not decode.  eng = None, or fewer than get_point_scan_min_terms() terms, runs on the host threads."""
    from .engine import sum_operands
    off, pidx, neg, points = sum_operands(off, points, pidx, neg)
    n_terms = int(off[-1])
    out = np.zeros((n_terms, 32), np.uint8)
    status = np.zeros(n_terms, np.uint8)
    _raise(lib().zkp_point_scan_batch(None if eng is None else eng._h, int(bool(exclusive)), len(off) - 1, _p(off), _p(pidx), _p(neg),
                                      _p(points) if len(points) else None, len(points), threads, _p(out), _p(status)), "zkp_point_scan_batch")
    return out, status


def set_point_scan_min_terms(n: int) -> None:
    """point_cumsum jobs on an engine with at least n terms run on the device (0: always; 2**64 - 1: never)"""
    lib().zkp_toolbox_set_point_scan_min_terms(n)


def get_point_scan_min_terms() -> int:
    return int(lib().zkp_toolbox_get_point_scan_min_terms())


# ---- bounded discrete logarithms to the basepoint (include/zkp_toolbox.h): m from encode(m B), m < 2**bits; eng = None is the host backend ----
def basepoint_dlog(eng, points, bits: int, threads: int = 0):
    """points [n][32] -> (k uint64 [n], status uint8 [n]): status 0 and encode(k B) == points[i] with k < 2**bits, 1 where the encoding does not
    decode, 2 where no k is in range (k = 0 for both).  bits in 1 .. 48.  Variable time: the duration depends on the logarithms."""
    from .engine import _u8
    points = _u8(points, 32)
    n = len(points)
    out = np.zeros(n, np.uint64)
    status = np.zeros(n, np.uint8)
    _raise(lib().zkp_basepoint_dlog_batch(None if eng is None else eng._h, n, _p(points), bits, _p(out), _p(status), threads), "zkp_basepoint_dlog_batch")
    return out, status


def point_dlog(eng, base, points, bits: int, signed: bool = False, threads: int = 0):
    """basepoint_dlog to the base with encoding `base` (32 bytes): points [n][32] -> (k [n], status uint8 [n]) with encode(k G) == points[i]; signed:
    k in [-2**(bits - 1), 2**(bits - 1)) as np.int64, else k < 2**bits as np.uint64.  On an engine the base takes one of the context's slots
    (Engine.prepare_dlog_point picks the size first; the default is 2**16 rows)."""
    from .engine import _base32, _u8
    points = _u8(points, 32)
    base = _base32(base)
    n = len(points)
    out = np.zeros(n, np.uint64)
    status = np.zeros(n, np.uint8)
    _raise(lib().zkp_point_dlog_batch(None if eng is None else eng._h, _p(base), n, _p(points), bits, 1 if signed else 0, _p(out), _p(status), threads),
           "zkp_point_dlog_batch")
    return (out.view(np.int64) if signed else out), status


def set_dlog_baby_bits(baby_bits: int) -> None:
    """the size of the host backend's baby-step table (2**baby_bits rows, 4 .. 22) for later basepoint_dlog calls"""
    _raise(lib().zkp_toolbox_set_dlog_baby_bits(baby_bits), "zkp_toolbox_set_dlog_baby_bits")


def get_dlog_baby_bits() -> int:
    return int(lib().zkp_toolbox_get_dlog_baby_bits())


def set_dlog_host_max_steps(steps: int) -> None:
    """calls whose host work n * (2**(bits - host baby_bits) + 128) -- giant steps, a point counting 128 for its decode and halving -- is at most
    `steps` per thread (threads counted up to 16) stay on the host threads even with an engine"""
    lib().zkp_toolbox_set_dlog_host_max_steps(steps)


def get_dlog_host_max_steps() -> int:
    return int(lib().zkp_toolbox_get_dlog_host_max_steps())


# ---- pipelines and device groups (include/zkp_toolbox.h, round 4) ------------------------------------------------------
def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array in pinned host memory (zkp_host_alloc): jobs copy from / to it without staging.  The memory is freed when
    the array (and every view of it) is gone."""
    hip = load_library()
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = ctypes.c_void_p()
    rc = hip.zkp_host_alloc(ctypes.byref(ptr), max(nbytes, 1))
    if rc != 0:
        _raise(rc, "zkp_host_alloc")

    class _Owner:
        def __init__(self, p):
            self.p = p

        def __del__(self):
            try:
                hip.zkp_host_free(self.p)
            except Exception:
                pass
    buf = (ctypes.c_uint8 * max(nbytes, 1)).from_address(ptr.value)
    buf._owner = _Owner(ptr)                                     # keeps the allocation alive as long as the ctypes buffer is
    return np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)


def pinned_copy(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class Job:
    """A submitted call of a Pipe.  wait() returns what the synchronous call returns; the arrays handed to submit (kept alive
    here) hold the outputs afterwards.  The C side holds pointers into those arrays until the job has been waited for, so a Job
    that is dropped un-waited waits in __del__, and Pipe.close() waits for every job it still has in flight first."""

    def __init__(self, handle, keep, outputs, kind, pipe=None):
        self._h, self._keep, self.outputs, self.kind = handle, keep, outputs, kind
        self.context = int(lib().zkp_job_context_index(handle))
        self._pipe = pipe                                   # (keeps the pipe alive as long as the job is)
        if pipe is not None:
            pipe._jobs.add(self)

    def done(self) -> bool:
        return self._h is None or bool(lib().zkp_job_done(self._h))

    def wait(self, raise_on_failure: bool = True):
        if self._h is None:
            raise RuntimeError("job already waited for")
        rc = lib().zkp_job_wait(self._h)
        self._h = None
        self.rc = rc
        if rc < 0 or (raise_on_failure and rc != 0):
            _raise(rc, "zkp_job_wait")
        return self.outputs

    def _retire(self) -> None:
        """wait without raising (drop / pipe shutdown): afterwards nothing on the C side names this job's arrays"""
        if self._h is not None:
            h, self._h = self._h, None
            self.rc = lib().zkp_job_wait(h)

    def __del__(self):
        try:
            if self._pipe is None or getattr(self._pipe, "_h", None):
                self._retire()
        except Exception:
            pass


class Pipe:
    """zkp_pipe: `contexts_per_device` engine contexts on each listed GPU; asynchronous jobs (submit_* -> Job) and synchronous
    calls sharded over all contexts (prove_batch, batch_verify, ...)."""

    def __init__(self, devices=(0,), contexts_per_device: int = 3):
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = lib().zkp_pipe_create(ctypes.byref(h), devs, len(devices), contexts_per_device)
        if rc != 0:
            _raise(rc, "zkp_pipe_create")
        self._h = h
        self._jobs = weakref.WeakSet()                      # submitted and not yet waited for

    def close(self):
        if getattr(self, "_h", None):
            for j in list(self._jobs):                      # their arrays are still named by the contexts' pending copies
                j._retire()
            lib().zkp_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def num_contexts(self) -> int:
        return int(lib().zkp_pipe_num_contexts(self._h))

    @property
    def jobs_in_flight(self) -> int:
        return int(lib().zkp_pipe_jobs_in_flight(self._h))

    def last_error(self) -> str:
        return lib().zkp_pipe_last_error(self._h).decode()

    def set_submit_threads(self, on: int) -> None:
        """zkp_pipe_set_submit_threads: 1 = asynchronous submits are carried out by one host thread per entry of the device list (the default of a
        pipe over several entries), 0 = by the caller's thread, -1 = default.  Only while no job is in flight."""
        rc = lib().zkp_pipe_set_submit_threads(self._h, int(on))
        if rc != 0:
            _raise(rc, "zkp_pipe_set_submit_threads")

    def set_profiling(self, on: bool) -> None:
        hip = load_library()
        for i in range(self.num_contexts):
            hip.zkp_ctx_set_profiling(lib().zkp_pipe_context(self._h, i), 1 if on else 0)

    def job_timing(self, context: int):
        """(ms of host -> device copies, kernels, device -> host copies) of the last job that finished on that context (profiling on)"""
        ms = (ctypes.c_float * 3)()
        load_library().zkp_ctx_job_timing(lib().zkp_pipe_context(self._h, context), ms)
        return tuple(float(x) for x in ms)

    def set_option(self, option: int, value: int, context: Optional[int] = None) -> None:
        """zkp_ctx_set_option on one context of the pipe, or on all of them"""
        hip = load_library()
        for i in ([context] if context is not None else range(self.num_contexts)):
            rc = hip.zkp_ctx_set_option(lib().zkp_pipe_context(self._h, i), option, value)
            if rc != 0:
                _raise(rc, "zkp_ctx_set_option")

    # -- asynchronous jobs ------------------------------------------------------------------------------------------
    @staticmethod
    def _ts(transcripts, n):
        """-> (array, flags): one 208-byte blob (shared) or [n][208]"""
        t = np.ascontiguousarray(transcripts, dtype=np.uint8)
        if t.shape == (TRANSCRIPT_BYTES,):
            return t, ZKP_JOB_SHARED_TRANSCRIPT
        if t.shape != (n, TRANSCRIPT_BYTES):
            raise ValueError("transcripts must be one blob [208] or [%d][208]" % n)
        return t, 0

    @staticmethod
    def _need(what, a, n_elems):
        """the C side reads n_elems elements: a shorter array would be an out-of-bounds read, not an error code"""
        if a is not None and np.asarray(a).size < n_elems:
            raise ValueError("%s has %d elements, the call reads %d" % (what, np.asarray(a).size, n_elems))

    def _submit(self, rc, h, what):
        if rc == ZKP_TB_PIPE_FULL:
            raise BlockingIOError("every context of the pipe has a job in flight")
        if rc != 0:
            _raise(rc, what)
        return h

    def submit_prove(self, st: Statement, n: int, transcripts, secrets, inst, common, entropy=None, want_transcripts=False, out=None,
                     inst_stride: Optional[int] = None) -> Job:
        """zkp_prove_batch_submit.  transcripts: one blob [208] (every proof starts from it) or [n][208].  out = optional dict of
        preallocated (e.g. pinned) arrays chal / resp / coms / ts.  -> Job whose outputs are (chal, resp, coms[, ts])."""
        ts, flags = self._ts(transcripts, n)
        self._need("secrets", secrets, n * st.m * 32)
        if not inst_stride:                       # (with a stride the caller passes a window into a larger array: its extent is the caller's business)
            self._need("inst", inst, st.ni * n * 32)
        self._need("common", common, st.ns * 32); self._need("entropy", entropy, n * 32)
        out = out or {}
        chal = out.get("chal") if out.get("chal") is not None else np.zeros((n, 32), np.uint8)
        resp = out.get("resp") if out.get("resp") is not None else np.zeros((n, st.m, 32), np.uint8)
        coms = out.get("coms") if out.get("coms") is not None else np.zeros((n, st.nc, 32), np.uint8)
        ts_out = (out.get("ts") if out.get("ts") is not None else np.zeros((n, TRANSCRIPT_BYTES), np.uint8)) if want_transcripts else None
        keep = [ts, np.ascontiguousarray(secrets), inst if inst_stride else np.ascontiguousarray(inst), np.ascontiguousarray(common),
                None if entropy is None else np.ascontiguousarray(entropy), chal, resp, coms, ts_out]
        h = ctypes.c_void_p()
        rc = lib().zkp_prove_batch_submit(self._h, st._h, n, flags, _p(keep[0]), _p(keep[1]), _p(keep[2]), inst_stride or n, _p(keep[3]), _p(keep[4]),
                                          _p(ts_out), _p(chal), _p(resp), _p(coms), ctypes.byref(h))
        self._submit(rc, h, "zkp_prove_batch_submit")
        return Job(h, keep + [st], (chal, resp, coms) + ((ts_out,) if want_transcripts else ()), "prove", self)

    def submit_batch_verify_many(self, st: Statement, n_batches: int, n_each: int, transcripts, inst, common, commitments, responses, weights16=None,
                                 want_transcripts=False, inst_stride: Optional[int] = None, weights_stride: Optional[int] = None) -> Job:
        """zkp_batch_verify_many_submit -> Job whose outputs are (verdicts[n_batches] (0 = Ok, 1 = VerificationFailure)[, ts])."""
        n = n_batches * n_each
        ts, flags = self._ts(transcripts, n)
        if not inst_stride:
            self._need("inst", inst, st.ni * n * 32)
        self._need("common", common, st.ns * 32); self._need("commitments", commitments, n * st.nc * 32); self._need("responses", responses, n * st.m * 32)
        if not weights_stride:
            self._need("weights16", weights16, st.nc * n * 16)
        verdicts = np.ones(n_batches, np.int32)
        ts_out = np.zeros((n, TRANSCRIPT_BYTES), np.uint8) if want_transcripts else None
        keep = [ts, inst if inst_stride else np.ascontiguousarray(inst), np.ascontiguousarray(common), np.ascontiguousarray(commitments),
                np.ascontiguousarray(responses), None if weights16 is None else (weights16 if weights_stride else np.ascontiguousarray(weights16)), verdicts, ts_out]
        h = ctypes.c_void_p()
        rc = lib().zkp_batch_verify_many_submit(self._h, st._h, n_batches, n_each, flags, _p(keep[0]), _p(keep[1]), inst_stride or n, _p(keep[2]), _p(keep[3]),
                                                _p(keep[4]), _p(keep[5]), weights_stride or n, _p(ts_out), _p(verdicts), ctypes.byref(h))
        self._submit(rc, h, "zkp_batch_verify_many_submit")
        return Job(h, keep + [st], (verdicts,) + ((ts_out,) if want_transcripts else ()), "batch_verify_many", self)

    def submit_verify_compact(self, st: Statement, n: int, transcripts, inst, common, challenges, responses, want_transcripts=False,
                              inst_stride: Optional[int] = None) -> Job:
        ts, flags = self._ts(transcripts, n)
        if not inst_stride:
            self._need("inst", inst, st.ni * n * 32)
        self._need("common", common, st.ns * 32); self._need("challenges", challenges, n * 32); self._need("responses", responses, n * st.m * 32)
        res = np.ones(n, np.uint8)
        ts_out = np.zeros((n, TRANSCRIPT_BYTES), np.uint8) if want_transcripts else None
        keep = [ts, inst if inst_stride else np.ascontiguousarray(inst), np.ascontiguousarray(common), np.ascontiguousarray(challenges),
                np.ascontiguousarray(responses), res, ts_out]
        h = ctypes.c_void_p()
        rc = lib().zkp_verify_compact_batch_submit(self._h, st._h, n, flags, _p(keep[0]), _p(keep[1]), inst_stride or n, _p(keep[2]), _p(keep[3]), _p(keep[4]),
                                                   _p(ts_out), _p(res), ctypes.byref(h))
        self._submit(rc, h, "zkp_verify_compact_batch_submit")
        return Job(h, keep + [st], (res,) + ((ts_out,) if want_transcripts else ()), "verify_compact", self)

    def submit_verify_batchable_each(self, st: Statement, n: int, transcripts, inst, common, commitments, responses, weights16=None,
                                     want_transcripts=False, inst_stride: Optional[int] = None) -> Job:
        ts, flags = self._ts(transcripts, n)
        if not inst_stride:
            self._need("inst", inst, st.ni * n * 32)
        self._need("common", common, st.ns * 32); self._need("commitments", commitments, n * st.nc * 32); self._need("responses", responses, n * st.m * 32)
        self._need("weights16", weights16, n * st.nc * 16)
        res = np.ones(n, np.uint8)
        ts_out = np.zeros((n, TRANSCRIPT_BYTES), np.uint8) if want_transcripts else None
        keep = [ts, inst if inst_stride else np.ascontiguousarray(inst), np.ascontiguousarray(common), np.ascontiguousarray(commitments),
                np.ascontiguousarray(responses), None if weights16 is None else np.ascontiguousarray(weights16), res, ts_out]
        h = ctypes.c_void_p()
        rc = lib().zkp_verify_batchable_each_submit(self._h, st._h, n, flags, _p(keep[0]), _p(keep[1]), inst_stride or n, _p(keep[2]), _p(keep[3]), _p(keep[4]),
                                                    _p(keep[5]), _p(ts_out), _p(res), ctypes.byref(h))
        self._submit(rc, h, "zkp_verify_batchable_each_submit")
        return Job(h, keep + [st], (res,) + ((ts_out,) if want_transcripts else ()), "verify_batchable_each", self)

    # -- synchronous calls sharded over every context (one host thread per listed device) ------------------------------
    def prove_batch(self, st: Statement, transcripts: np.ndarray, secrets, inst, common, entropy=None):
        n = len(transcripts)
        _check_batch_shapes(st, n, inst, common, None, secrets)
        chal = np.zeros((n, 32), np.uint8)
        resp = np.zeros((n, st.m, 32), np.uint8)
        coms = np.zeros((n, st.nc, 32), np.uint8)
        rc = lib().zkp_pipe_prove_batch(self._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(secrets)), _p(np.ascontiguousarray(inst)),
                                        _p(np.ascontiguousarray(common)), _p(None if entropy is None else np.ascontiguousarray(entropy)), _p(chal), _p(resp), _p(coms))
        _raise(rc, "zkp_pipe_prove_batch")
        return chal, resp, coms

    def verify_compact_batch(self, st, transcripts, inst, common, challenges, responses) -> np.ndarray:
        n = len(transcripts)
        _check_batch_shapes(st, n, inst, common, None, responses)
        res = np.ones(n, np.uint8)
        rc = lib().zkp_pipe_verify_compact_batch(self._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                                 _p(np.ascontiguousarray(challenges)), _p(np.ascontiguousarray(responses)), _p(res))
        _raise(rc, "zkp_pipe_verify_compact_batch")
        return res

    def verify_batchable_each(self, st, transcripts, inst, common, commitments, responses, weights16=None) -> np.ndarray:
        n = len(transcripts)
        _check_batch_shapes(st, n, inst, common, commitments, responses, weights16, per_proof_weights=True)
        res = np.ones(n, np.uint8)
        rc = lib().zkp_pipe_verify_batchable_each(self._h, st._h, n, _p(transcripts), _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                                  _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                                  _p(None if weights16 is None else np.ascontiguousarray(weights16)), _p(res))
        _raise(rc, "zkp_pipe_verify_batchable_each")
        return res

    def batch_verify(self, st, transcripts, inst, common, commitments, responses, weights16=None) -> None:
        """Raises VerificationFailure unless every range of the batch verifies (host AND of the per-context verdicts)."""
        n = len(commitments)
        _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
        rc = lib().zkp_pipe_batch_verify(self._h, st._h, n, len(transcripts), _p(transcripts), _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                         _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                         _p(None if weights16 is None else np.ascontiguousarray(weights16)))
        _raise(rc, "zkp_pipe_batch_verify")

    def batch_verify_many(self, st, n_batches: int, transcripts, inst, common, commitments, responses, weights16=None) -> np.ndarray:
        n = len(commitments)
        if n_batches <= 0 or n % n_batches:
            raise ValueError("the number of proofs must be a positive multiple of n_batches")
        _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
        verdicts = np.ones(n_batches, np.int32)
        rc = lib().zkp_pipe_batch_verify_many(self._h, st._h, n_batches, n // n_batches, len(transcripts), _p(transcripts), _p(np.ascontiguousarray(inst)),
                                              _p(np.ascontiguousarray(common)), _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                              _p(None if weights16 is None else np.ascontiguousarray(weights16)), _p(verdicts))
        _raise(rc, "zkp_pipe_batch_verify_many")
        return verdicts

    def batch_verify_locate(self, st, transcripts, inst, common, commitments, responses, weights16=None):
        n = len(commitments)
        _check_batch_shapes(st, n, inst, common, commitments, responses, weights16)
        res = np.ones(n, np.uint8)
        rc = lib().zkp_pipe_batch_verify_locate(self._h, st._h, n, len(transcripts), _p(transcripts), _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                                _p(np.ascontiguousarray(commitments)), _p(np.ascontiguousarray(responses)),
                                                _p(None if weights16 is None else np.ascontiguousarray(weights16)), _p(res))
        if rc not in (0, 1):
            _raise(rc, "zkp_pipe_batch_verify_locate")
        return rc == 0, res


def prove_phase_a(st, transcripts, secrets, inst, common, entropy, threads: int = 0):
    n = len(transcripts)
    blind = np.zeros((n, st.m, 32), np.uint8)
    off = np.zeros(n * st.nc + 1, np.uint32)
    sc = np.zeros((n * st.terms, 32), np.uint8)
    pidx = np.zeros(n * st.terms, np.uint32)
    rc = lib().zkp_prove_phase_a(st._h, n, _p(transcripts), _p(np.ascontiguousarray(secrets)),
                                 _p(np.ascontiguousarray(inst)), _p(np.ascontiguousarray(common)),
                                 _p(np.ascontiguousarray(entropy)), threads, _p(blind), _p(off), _p(sc), _p(pidx))
    _raise(rc, "zkp_prove_phase_a")
    return blind, off, sc, pidx


def prove_phase_b(st, transcripts, secrets, blindings, commitments, threads: int = 0):
    n = len(transcripts)
    chal = np.zeros((n, 32), np.uint8)
    resp = np.zeros((n, st.m, 32), np.uint8)
    rc = lib().zkp_prove_phase_b(st._h, n, _p(transcripts), _p(np.ascontiguousarray(secrets)),
                                 _p(np.ascontiguousarray(blindings)), _p(np.ascontiguousarray(commitments)), threads, _p(chal), _p(resp))
    _raise(rc, "zkp_prove_phase_b")
    return chal, resp


# ---- the reference's object API (one proof at a time; the batch functions do the work) ------------
@dataclass(frozen=True)
class ScalarVar:
    idx: int


@dataclass(frozen=True)
class PointVar:
    idx: int


def _enc(e) -> bytes:
    e = bytes(e) if not isinstance(e, np.ndarray) else e.tobytes()
    assert len(e) == 32
    return e


class Prover:
    """toolbox::prover::Prover (src/toolbox/prover.rs).  Points are supplied as encodings."""

    def __init__(self, proof_label: bytes, transcript: Transcript, engine: Engine):
        self._st = Statement(proof_label)
        self._t = transcript
        self._eng = engine
        self._scalars: List[bytes] = []
        self._points: List[bytes] = []

    def allocate_scalar(self, label: bytes, assignment) -> ScalarVar:
        self._scalars.append(scalar_bytes(assignment))
        return ScalarVar(self._st.add_secret(label))

    def allocate_point(self, label: bytes, assignment) -> Tuple[PointVar, bytes]:
        e = _enc(assignment)
        self._points.append(e)
        return PointVar(self._st.add_point(label, False)), e

    def constrain(self, lhs: PointVar, linear_combination: Sequence[Tuple[ScalarVar, PointVar]]) -> None:
        self._st.constrain(lhs.idx, [(s.idx, p.idx) for s, p in linear_combination])

    def _prove(self, entropy: Optional[bytes]):
        ts = self._t.state.reshape(1, -1).copy()
        secrets = np.frombuffer(b"".join(self._scalars), np.uint8).reshape(1, -1, 32) if self._scalars else np.zeros((1, 0, 32), np.uint8)
        inst = np.frombuffer(b"".join(self._points), np.uint8).reshape(-1, 1, 32) if self._points else np.zeros((0, 1, 32), np.uint8)
        ent = None if entropy is None else np.frombuffer(entropy, np.uint8).reshape(1, 32)
        chal, resp, coms = prove_batch(self._eng, self._st, ts, secrets, inst, np.zeros((0, 32), np.uint8), ent, threads=1)
        self._t.state[:] = ts[0]
        return chal[0].tobytes(), [r.tobytes() for r in resp[0]], [c.tobytes() for c in coms[0]]

    def prove_compact(self, entropy: Optional[bytes] = None) -> CompactProof:
        c, r, _ = self._prove(entropy)
        return CompactProof(c, r)

    def prove_batchable(self, entropy: Optional[bytes] = None) -> BatchableProof:
        _, r, k = self._prove(entropy)
        return BatchableProof(k, r)


class Verifier:
    """toolbox::verifier::Verifier (src/toolbox/verifier.rs)."""

    def __init__(self, proof_label: bytes, transcript: Transcript, engine: Engine):
        self._st = Statement(proof_label)
        self._t = transcript
        self._eng = engine
        self._points: List[bytes] = []

    def allocate_scalar(self, label: bytes) -> ScalarVar:
        return ScalarVar(self._st.add_secret(label))

    def allocate_point(self, label: bytes, assignment) -> PointVar:
        e = _enc(assignment)
        if e == bytes(32):                      # validate_and_append_point_var, mod.rs:191-193
            raise VerificationFailure()
        self._points.append(e)
        return PointVar(self._st.add_point(label, False))

    def constrain(self, lhs: PointVar, linear_combination) -> None:
        self._st.constrain(lhs.idx, [(s.idx, p.idx) for s, p in linear_combination])

    def _inst(self):
        return np.frombuffer(b"".join(self._points), np.uint8).reshape(-1, 1, 32) if self._points else np.zeros((0, 1, 32), np.uint8)

    def verify_compact(self, proof: CompactProof) -> None:
        if len(proof.responses) != self._st.m:                          # verifier.rs:82-84
            raise VerificationFailure()
        ts = self._t.state.reshape(1, -1).copy()
        resp = np.frombuffer(b"".join(proof.responses), np.uint8).reshape(1, -1, 32) if proof.responses else np.zeros((1, 0, 32), np.uint8)
        res = verify_compact_batch(self._eng, self._st, ts, self._inst(), np.zeros((0, 32), np.uint8),
                                   np.frombuffer(proof.challenge, np.uint8).reshape(1, 32), resp, threads=1)
        self._t.state[:] = ts[0]
        if res[0]:
            raise VerificationFailure()

    def verify_batchable(self, proof: BatchableProof, weights: Optional[Sequence[int]] = None) -> None:
        if len(proof.responses) != self._st.m or len(proof.commitments) != self._st.nc:     # verifier.rs:125-131
            raise VerificationFailure()
        ts = self._t.state.reshape(1, -1).copy()
        resp = np.frombuffer(b"".join(proof.responses), np.uint8).reshape(1, -1, 32) if proof.responses else np.zeros((1, 0, 32), np.uint8)
        coms = np.frombuffer(b"".join(proof.commitments), np.uint8).reshape(1, -1, 32) if proof.commitments else np.zeros((1, 0, 32), np.uint8)
        w = None if weights is None else np.frombuffer(b"".join(int(x).to_bytes(16, "little") for x in weights), np.uint8).reshape(1, -1, 16)
        res = verify_batchable_each(self._eng, self._st, ts, self._inst(), np.zeros((0, 32), np.uint8), coms, resp, w, threads=1)
        self._t.state[:] = ts[0]
        if res[0]:
            raise VerificationFailure()


class BatchVerifier:
    """toolbox::batch_verifier::BatchVerifier (src/toolbox/batch_verifier.rs)."""

    def __init__(self, proof_label: bytes, batch_size: int, transcripts: Sequence[Transcript], engine: Engine):
        if len(transcripts) != batch_size:                              # batch_verifier.rs:72-74
            raise BatchSizeMismatch()
        self._st = Statement(proof_label)
        self._n = batch_size
        self._ts = list(transcripts)
        self._eng = engine
        self._static: List[bytes] = []
        self._instance: List[List[bytes]] = []

    def allocate_scalar(self, label: bytes) -> ScalarVar:
        return ScalarVar(self._st.add_secret(label))

    def allocate_static_point(self, label: bytes, assignment) -> PointVar:
        e = _enc(assignment)
        if e == bytes(32):
            raise VerificationFailure()
        self._static.append(e)
        return PointVar(self._st.add_point(label, True))

    def allocate_instance_point(self, label: bytes, assignments: Sequence) -> PointVar:
        if len(assignments) != self._n:                                 # batch_verifier.rs:120-122
            raise BatchSizeMismatch()
        es = [_enc(a) for a in assignments]
        if any(e == bytes(32) for e in es):
            raise VerificationFailure()
        self._instance.append(es)
        return PointVar(self._st.add_point(label, False))

    def constrain(self, lhs: PointVar, linear_combination) -> None:
        self._st.constrain(lhs.idx, [(s.idx, p.idx) for s, p in linear_combination])

    def verify_batchable(self, proofs: Sequence[BatchableProof], weights: Optional[Sequence[Sequence[int]]] = None) -> None:
        if len(proofs) != self._n:                                      # batch_verifier.rs:138-140
            raise BatchSizeMismatch()
        for p in proofs:                                                # batch_verifier.rs:142-149
            if len(p.commitments) != self._st.nc or len(p.responses) != self._st.m:
                raise VerificationFailure()
        n = self._n
        ts = _transcripts_array(self._ts)
        inst = np.frombuffer(b"".join(e for row in self._instance for e in row), np.uint8).reshape(-1, n, 32) if self._instance else np.zeros((0, n, 32), np.uint8)
        common = np.frombuffer(b"".join(self._static), np.uint8).reshape(-1, 32) if self._static else np.zeros((0, 32), np.uint8)
        coms = np.frombuffer(b"".join(c for p in proofs for c in p.commitments), np.uint8).reshape(n, -1, 32) if n and self._st.nc else np.zeros((n, 0, 32), np.uint8)
        resp = np.frombuffer(b"".join(r for p in proofs for r in p.responses), np.uint8).reshape(n, -1, 32) if n and self._st.m else np.zeros((n, 0, 32), np.uint8)
        w = None if weights is None else np.frombuffer(b"".join(int(x).to_bytes(16, "little") for row in weights for x in row), np.uint8).reshape(-1, n, 16)
        try:
            batch_verify(self._eng, self._st, ts, inst, common, coms, resp, w, batch_size=n)
        finally:
            _store_transcripts(self._ts, ts)


# ---- define_proof! -----------------------------------------------------------------------------------
class ProofModule:
    """What `define_proof!` generates (src/macros.rs:124-370): a statement with fixed labels and allocation
    order (secrets, instance points, common points) and the five entry points."""

    def __init__(self, name: str, label: bytes, secrets: Sequence[str], instance: Sequence[str], common: Sequence[str],
                 constraints: Sequence[Tuple[str, Sequence[Tuple[str, str]]]]):
        self.name, self.label = name, label
        self.secrets, self.instance, self.common = list(secrets), list(instance), list(common)
        self.constraints = [(l, list(lc)) for l, lc in constraints]
        self.statement = Statement(label)
        sv = {n: self.statement.add_secret(n.encode()) for n in self.secrets}                # macros.rs:215-222
        pv = {n: self.statement.add_point(n.encode(), False) for n in self.instance}         # macros.rs:229-235
        pv.update({n: self.statement.add_point(n.encode(), True) for n in self.common})      # macros.rs:236-242
        for lhs, lc in self.constraints:                                                    # macros.rs:159-170
            self.statement.constrain(pv[lhs], [(sv[s], pv[p]) for s, p in lc])

    # -- array helpers ----------------------------------------------------------------------------
    def pack(self, secrets: Sequence[Dict[str, object]], points: Sequence[Dict[str, bytes]]):
        """list of per-proof dicts -> (secrets[N][m][32], inst[ni][N][32], common[ns][32])"""
        n = len(points)
        sec = np.frombuffer(b"".join(scalar_bytes(s[k]) for s in secrets for k in self.secrets), np.uint8).reshape(n, len(self.secrets), 32) if secrets else None
        inst = np.frombuffer(b"".join(_enc(p[k]) for k in self.instance for p in points), np.uint8).reshape(len(self.instance), n, 32)
        common = np.frombuffer(b"".join(_enc(points[0][k]) for k in self.common), np.uint8).reshape(len(self.common), 32)
        return sec, inst, common

    def prove_compact(self, eng, transcript: Transcript, secrets: Dict[str, object], points: Dict[str, bytes], entropy=None) -> CompactProof:
        c, r, _ = self._prove(eng, transcript, secrets, points, entropy)
        return CompactProof(c, r)

    def prove_batchable(self, eng, transcript: Transcript, secrets, points, entropy=None) -> BatchableProof:
        _, r, k = self._prove(eng, transcript, secrets, points, entropy)
        return BatchableProof(k, r)

    def _prove(self, eng, transcript, secrets, points, entropy):
        sec, inst, common = self.pack([secrets], [points])
        ts = transcript.state.reshape(1, -1).copy()
        ent = None if entropy is None else np.frombuffer(entropy, np.uint8).reshape(1, 32)
        chal, resp, coms = prove_batch(eng, self.statement, ts, sec, inst, common, ent, threads=1)
        transcript.state[:] = ts[0]
        return chal[0].tobytes(), [x.tobytes() for x in resp[0]], [x.tobytes() for x in coms[0]]

    def verify_compact(self, eng, proof: CompactProof, transcript: Transcript, points: Dict[str, bytes]) -> None:
        if any(_enc(points[k]) == bytes(32) for k in self.instance + self.common) or len(proof.responses) != len(self.secrets):
            raise VerificationFailure()
        _, inst, common = self.pack([], [points])
        ts = transcript.state.reshape(1, -1).copy()
        res = verify_compact_batch(eng, self.statement, ts, inst, common, np.frombuffer(proof.challenge, np.uint8).reshape(1, 32),
                                   np.frombuffer(b"".join(proof.responses), np.uint8).reshape(1, -1, 32), threads=1)
        transcript.state[:] = ts[0]
        if res[0]:
            raise VerificationFailure()

    def verify_batchable(self, eng, proof: BatchableProof, transcript: Transcript, points: Dict[str, bytes], weights=None) -> None:
        if len(proof.responses) != len(self.secrets) or len(proof.commitments) != len(self.constraints):
            raise VerificationFailure()
        _, inst, common = self.pack([], [points])
        ts = transcript.state.reshape(1, -1).copy()
        w = None if weights is None else np.frombuffer(b"".join(int(x).to_bytes(16, "little") for x in weights), np.uint8).reshape(1, -1, 16)
        res = verify_batchable_each(eng, self.statement, ts, inst, common,
                                    np.frombuffer(b"".join(proof.commitments), np.uint8).reshape(1, -1, 32),
                                    np.frombuffer(b"".join(proof.responses), np.uint8).reshape(1, -1, 32), w, threads=1)
        transcript.state[:] = ts[0]
        if res[0]:
            raise VerificationFailure()

    def batch_verify(self, eng, proofs: Sequence[BatchableProof], transcripts: Sequence[Transcript],
                     instance_points: Dict[str, Sequence[bytes]], common_points: Dict[str, bytes], weights=None, threads: int = 0) -> None:
        n = len(proofs)
        if len(transcripts) != n:
            raise BatchSizeMismatch()
        for k in self.instance:
            if len(instance_points[k]) != n:
                raise BatchSizeMismatch()
        for p in proofs:                                                # batch_verifier.rs:142-149
            if len(p.commitments) != len(self.constraints) or len(p.responses) != len(self.secrets):
                raise VerificationFailure()
        ts = _transcripts_array(transcripts)
        inst = np.frombuffer(b"".join(_enc(e) for k in self.instance for e in instance_points[k]), np.uint8).reshape(len(self.instance), n, 32)
        common = np.frombuffer(b"".join(_enc(common_points[k]) for k in self.common), np.uint8).reshape(len(self.common), 32)
        coms = np.frombuffer(b"".join(c for p in proofs for c in p.commitments), np.uint8).reshape(n, len(self.constraints), 32)
        resp = np.frombuffer(b"".join(r for p in proofs for r in p.responses), np.uint8).reshape(n, len(self.secrets), 32)
        w = None if weights is None else np.frombuffer(b"".join(int(x).to_bytes(16, "little") for row in weights for x in row), np.uint8).reshape(len(self.constraints), n, 16)
        try:
            batch_verify(eng, self.statement, ts, inst, common, coms, resp, w, threads=threads, batch_size=n)
        finally:
            _store_transcripts(transcripts, ts)


def define_proof(name, label, secrets, instance, common, constraints) -> ProofModule:
    return ProofModule(name, label if isinstance(label, bytes) else label.encode(), secrets, instance, common, constraints)


def dleq_module() -> ProofModule:
    """define_proof! {dleq, "DLEQ proof", (x), (A, B, H), (G) : A = (x * G), B = (x * H)}  (benches/zkp.rs:49)"""
    return define_proof("dleq", b"DLEQ proof", ["x"], ["A", "B", "H"], ["G"], [("A", [("x", "G")]), ("B", [("x", "H")])])


def cmz_module(n: int = 10) -> ProofModule:
    """cred_show_10 (benches/zkp.rs:27-46)."""
    ms = [f"m_{i}" for i in range(1, n + 1)]
    zs = [f"z_{i}" for i in range(1, n + 1)]
    cs = [f"C_{i}" for i in range(1, n + 1)]
    xs = [f"X_{i}" for i in range(1, n + 1)]
    cons = [(cs[i], [(ms[i], "P"), (zs[i], "A")]) for i in range(n)]
    cons.append(("V", [(ms[i], xs[i]) for i in range(n)] + [("minus_z_Q", "Q")]))
    return define_proof(f"cred_show_{n}", f"CMZ cred show n={n}".encode(), ms + zs + ["minus_z_Q"], cs + ["P", "Q", "V"], xs + ["A", "B"], cons)

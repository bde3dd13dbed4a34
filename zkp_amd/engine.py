"""ctypes binding of the C-ABI library (include/zkp_mi355x.h -> zkp_amd/libzkp_mi355x.so).

This is plumbing only: every function forwards to the HIP library and raises if the library or a
GPU is missing -- there is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from . import cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzkp_mi355x.so")
TESTHOOKS_LIB_PATH = os.path.join(_HERE, "libzkp_mi355x_testhooks.so")     # -DZKP_BUILD_TEST_HOOKS build (tests / A-B tools)
ZKP_TESTOPT_DUMMY_LAUNCHES, ZKP_TESTOPT_GENERIC_CLASSIFIER, ZKP_TESTOPT_WAVE_CYCLES, ZKP_TESTOPT_PIP_MERGE, ZKP_TESTOPT_VOUCH_REDUCED = 1001, 1002, 1003, 1004, 1005
ZKP_TESTOPT_PIP_RUN_CAP = 1006
ZKP_OPT_CT_LOOKUP, ZKP_OPT_EACH_STRAUS, ZKP_OPT_LADDER_INTERLEAVE = 9, 10, 11
ZKP_OPT_CT_MASKED_SCANS = ZKP_OPT_CT_LOOKUP           # the round-3 name (value 1 = masked scans)
ZKP_CT_LOOKUP_XBAR, ZKP_CT_LOOKUP_SCAN, ZKP_CT_LOOKUP_LDS = 0, 1, 2
ZKP_OPT_WS_LIMIT_BYTES, ZKP_OPT_JOB_DEFER_D2H, ZKP_OPT_SYNC_SCHEDULE, ZKP_OPT_TRANSCRIPT_STEPS, ZKP_OPT_COMB_SPLIT, ZKP_OPT_JOINT_LADDER = 12, 13, 14, 15, 16, 17

ZKP_VARTIME = 0
ZKP_CT = 1
ZKP_RNG_SCALARS = 0      # zkp_transcripts_witness_rng: count x Scalar::random
ZKP_RNG_BYTES = 1        # ... or one fill_bytes(count)
ZKP_PT_ADD, ZKP_PT_SUB = 0, 1               # zkp_add_points' op
ZKP_SC_SUM, ZKP_SC_PRODUCT, ZKP_SC_DOT = 0, 1, 2     # zkp_sc_reduce's op
ZKP_SCAN_INCLUSIVE, ZKP_SCAN_EXCLUSIVE = 0, 1        # zkp_sc_scan's and zkp_scan_points' mode
ZKP_DLOG_FOUND, ZKP_DLOG_INVALID, ZKP_DLOG_NOT_FOUND = 0, 1, 2      # zkp_dlog_base's status
ZKP_DLOG_SLOTS, ZKP_DLOG_SIGNED = 8, 1           # zkp_ctx_prepare_dlog_point's slots, zkp_dlog_point's flag
ZKP_OPT_BATCH_ENCODE_MIN = 1
(ZKP_OPT_COMB_TEETH, ZKP_OPT_CT_SINGLE_USE_TABLES, ZKP_OPT_TRANSCRIPT_LANES, ZKP_OPT_DEV_OVERLAP, ZKP_OPT_GROUPED_COMB, ZKP_OPT_TABLES_LANE,
 ZKP_OPT_FUSE_TABLES_TRANSCRIPT) = 2, 3, 4, 5, 6, 7, 8
K_NAMES = ("decode", "terms", "reduce", "sort", "bucket", "combine", "transcript", "scalars", "tables")

EXPORTS = tuple(cabi.signatures("zkp_mi355x.h"))
TEST_HOOK_EXPORTS = tuple(cabi.signatures("zkp_mi355x.h", test_hooks=True))      # only in libzkp_mi355x_testhooks.so


class ZkpError(RuntimeError):
    pass


_lib = None
_hooks_lib = None


def load_library(test_hooks: bool = False) -> ctypes.CDLL:
    """dlopen the HIP library, every function typed from include/zkp_mi355x.h; raises (never falls back) when it has not been built.
    test_hooks = the -DZKP_BUILD_TEST_HOOKS build of the same sources (a second, independent copy of the library: its contexts must not
    be handed to libzkp_toolbox.so), its hook section typed too."""
    global _lib, _hooks_lib
    if test_hooks and _hooks_lib is not None:
        return _hooks_lib
    if not test_hooks and _lib is not None:
        return _lib
    path = TESTHOOKS_LIB_PATH if test_hooks else LIB_PATH
    if not os.path.exists(path):
        raise ZkpError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = cabi.bind(cabi.bind(cabi.bind(ctypes.CDLL(path), "zkp_mi355x.h", test_hooks), "zkp_or_mi355x.h"), "zkp_or_batch_mi355x.h")
    if test_hooks:
        _hooks_lib = lib
    else:
        _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise ZkpError(f"{what} failed with code {rc}: {load_library().zkp_last_error().decode()}")


def _u8(a, shape_last: int) -> np.ndarray:
    if len(a) == 0:
        return np.zeros((0, shape_last), np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2 or a.shape[1] != shape_last:
        raise ValueError(f"expected uint8 array of shape [n][{shape_last}], got {a.shape}")
    return a


def _base32(base) -> np.ndarray:
    """one encoding, bytes or a uint8 row, as a contiguous uint8 [32]"""
    a = np.frombuffer(bytes(base), np.uint8) if isinstance(base, (bytes, bytearray)) else np.ascontiguousarray(base, dtype=np.uint8).reshape(-1)
    if a.shape != (32,):
        raise ValueError(f"expected one encoding of 32 bytes, got {a.shape}")
    return a.copy()


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def messages_csr(messages) -> Tuple[np.ndarray, np.ndarray]:
    """A list of byte strings as a CSR batch: (data uint8, offsets uint64 [n + 1]), message i = data[offsets[i]:offsets[i + 1]].  data
    has at least one byte, so that its pointer is never NULL."""
    msgs = [bytes(m) for m in messages]
    offsets = np.zeros(len(msgs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
    return data, offsets


def ragged_blocks(transcripts) -> Tuple[np.ndarray, np.ndarray]:
    """(test-hook build, no GPU needed) the class grouping the _ragged calls launch for transcripts [N][208]: (idx [N] = proof indices
    sorted stably by class, blocks [n][3] = (class, first, count) per wavefront, classes in order of first appearance)."""
    lib = load_library(test_hooks=True)
    ts = _u8(transcripts, 208)
    idx = np.zeros(len(ts), np.uint32)
    cap = len(ts) + 1
    blocks = np.zeros((cap, 3), np.uint32)
    n = lib.zkp_debug_ragged_blocks(_ptr(ts), len(ts), _ptr(idx), _ptr(blocks), cap)
    if n < 0:
        _check(n, "zkp_debug_ragged_blocks")
    return idx, blocks[:n]


def _csr_args(data, offsets) -> Tuple[np.ndarray, np.ndarray]:
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if len(offsets) < 1:
        raise ValueError("offsets must hold n + 1 entries")
    if len(offsets) > 1 and (np.any(offsets[1:] < offsets[:-1]) or int(offsets[-1]) > len(data)):
        raise ValueError("offsets must be non-decreasing and end within data")
    if len(data) == 0:
        data = np.zeros(1, np.uint8)
    return data, offsets


def _blobs(transcripts, n: int) -> np.ndarray:
    ts = transcripts
    if not (isinstance(ts, np.ndarray) and ts.dtype == np.uint8 and ts.shape == (n, 208) and ts.flags["C_CONTIGUOUS"]):
        raise ValueError("transcripts must be a C-contiguous uint8 array of shape [N][208] (they advance in place)")
    return ts


def strobe_pos_after_append(strobe_pos: int, label_len: int, msg_len: int) -> int:
    """zkp_strobe_pos_after_append (no GPU): the position word pos | pos_begin << 8 | cur_flags << 16 of a transcript after one
    append_message with a label of label_len and a message of msg_len bytes, from its position word before"""
    return int(load_library().zkp_strobe_pos_after_append(strobe_pos, label_len, msg_len))



def reduce_operands(op: int, off, a, aidx=None, b=None, bidx=None):
    """The operands of a segmented scalar fold as C-contiguous arrays: (off u32 [n_out + 1], a u8 [n_a][32], aidx u32 [T] or None, b or None,
    bidx or None).  Shapes only: the values are the library's to check."""
    off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
    if len(off) < 1:
        raise ValueError("off must hold n_out + 1 entries")
    n_terms = int(off[-1])

    def operand(x, idx, name):
        x = _u8(x, 32)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
            if len(idx) != n_terms:
                raise ValueError(f"{name}idx must hold off[-1] entries")
            if len(idx) == 0:
                idx = np.zeros(1, np.uint32)                    # never a NULL pointer for an index list that was given
        if len(x) == 0:
            x = np.zeros((0, 32), np.uint8)
        return x, idx

    a, aidx = operand(a, aidx, "a")
    if op == ZKP_SC_DOT:
        if b is None:
            raise ValueError("ZKP_SC_DOT needs b")
        b, bidx = operand(b, bidx, "b")
    elif b is not None or bidx is not None:
        raise ValueError("b and bidx belong to ZKP_SC_DOT")
    return off, a, aidx, b, bidx


def scalar_operands(a, b, c=None):
    """The operands of a * b + c as (n, (a, stride), (b, stride), (c, stride)): uint8 [n][32] has stride 1, shape (32,) or (1, 32) is one
    scalar for every row (stride 0); all three shared gives n = 1; c = None stays None."""
    ops = []
    for x in (a, b, c):
        if x is None:
            ops.append(None)
            continue
        x = np.ascontiguousarray(x, dtype=np.uint8)
        if x.shape == (32,):
            x = x.reshape(1, 32)
        if x.ndim != 2 or x.shape[1] != 32:
            raise ValueError(f"expected uint8 array of shape [n][32] or (32,), got {x.shape}")
        ops.append(x)
    if ops[0] is None or ops[1] is None:
        raise ValueError("a and b are required")
    sizes = {len(x) for x in ops if x is not None and len(x) != 1}
    if len(sizes) > 1:
        raise ValueError(f"operands of different lengths: {sorted(sizes)}")
    n = sizes.pop() if sizes else 1
    return (n,) + tuple((x, 0 if x is None or (len(x) == 1 and n != 1) else 1) for x in ops)


def mul_operands(scalars, points):
    """The operands of scalars * points as (n, (scalars, stride), (points, stride)): uint8 [n][32] has stride 1, shape (32,) or (1, 32) is one
    operand for every row (stride 0); both shared gives n = 1"""
    n, (s, ss), (p, ps), _ = scalar_operands(scalars, points)
    return n, (s, ss), (p, ps)


def sum_operands(off, points, pidx, neg):
    """The arrays of a segmented sum as the C ABI takes them: off uint32 [n_sums + 1], pidx uint32 [T] or None, neg uint8 [T] (0 / 1) or None,
    points uint8 [n_points][32]; lengths that disagree with off[-1] raise"""
    off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
    if len(off) < 1:
        raise ValueError("off must hold n_sums + 1 entries")
    n_terms = int(off[-1])
    points = _u8(points, 32)
    if pidx is not None:
        pidx = np.ascontiguousarray(pidx, dtype=np.uint32).reshape(-1)
        if len(pidx) != n_terms:
            raise ValueError("pidx length must equal off[-1]")
    if neg is not None:
        neg = np.ascontiguousarray(np.asarray(neg) != 0, dtype=np.uint8).reshape(-1)
        if len(neg) != n_terms:
            raise ValueError("neg length must equal off[-1]")
    return off, pidx, neg, points


class Engine:
    """One context on one GPU (HIP device ordinal `device`)."""

    def __init__(self, device: int = 0, test_hooks: bool = False):
        self._lib = load_library(test_hooks)
        self.test_hooks = test_hooks
        h = ctypes.c_void_p()
        _check(self._lib.zkp_ctx_create(ctypes.byref(h), device), "zkp_ctx_create")
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.zkp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def version(self) -> str:
        return self._lib.zkp_version().decode()

    def _need_hooks(self, fn: str) -> None:
        if not self.test_hooks:
            raise ZkpError(f"{fn} exists in the test-hook build only: Engine(device, test_hooks=True)")

    # ---- host-buffer entry points (numpy) ---------------------------------------------------
    def msm_many(self, off: Sequence[int], scalars, pidx: Sequence[int], points, flags: int = ZKP_VARTIME
                 ) -> Tuple[np.ndarray, np.ndarray]:
        """CSR batch of small MSMs -> (out[n_msm][32], status[n_msm])."""
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n_msm = len(off) - 1
        pidx = np.ascontiguousarray(pidx, dtype=np.uint32)
        n_terms = int(off[-1]) if n_msm >= 0 and len(off) else 0
        scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
        points = _u8(points, 32)
        if len(scalars) != n_terms or len(pidx) != n_terms:
            raise ValueError("scalars / pidx length must equal off[-1]")
        out = np.zeros((max(n_msm, 0), 32), np.uint8)
        status = np.zeros(max(n_msm, 0), np.uint8)
        _check(self._lib.zkp_msm_many(self._h, n_msm, _ptr(off), _ptr(scalars), _ptr(pidx), _ptr(points),
                                      len(points), flags, _ptr(out), _ptr(status)), "zkp_msm_many")
        return out, status

    def msm_optional(self, scalars, points) -> Optional[bytes]:
        """optional_multiscalar_mul: encoding of sum s_i * decode(P_i), or None if a decode fails."""
        scalars, points = _u8(scalars, 32), _u8(points, 32)
        if len(scalars) != len(points):
            raise ValueError("scalars and points must have equal length")
        out = np.zeros(32, np.uint8)
        st = ctypes.c_int(1)
        _check(self._lib.zkp_msm_optional(self._h, len(scalars), _ptr(scalars), _ptr(points), _ptr(out), ctypes.byref(st)),
               "zkp_msm_optional")
        return None if st.value else out.tobytes()

    def decode_check(self, points, want_coords: bool = False):
        points = _u8(points, 32)
        status = np.zeros(len(points), np.uint8)
        xyzt = np.zeros((len(points), 128), np.uint8) if want_coords else None
        _check(self._lib.zkp_decode_check(self._h, len(points), _ptr(points), _ptr(status), _ptr(xyzt)), "zkp_decode_check")
        return (status, xyzt) if want_coords else status

    def encode_many(self, xyzt) -> np.ndarray:
        xyzt = _u8(xyzt, 128)
        out = np.zeros((len(xyzt), 32), np.uint8)
        _check(self._lib.zkp_encode_many(self._h, len(xyzt), _ptr(xyzt), _ptr(out)), "zkp_encode_many")
        return out

    def from_uniform_bytes(self, inp) -> np.ndarray:
        """RistrettoPoint::from_uniform_bytes (RFC 9496 section 4.3.4) of every 64-byte row: [n][64] -> canonical encodings [n][32]"""
        inp = _u8(inp, 64)
        out = np.zeros((len(inp), 32), np.uint8)
        _check(self._lib.zkp_from_uniform_bytes(self._h, len(inp), _ptr(inp), _ptr(out)), "zkp_from_uniform_bytes")
        return out

    def hash_from_bytes_sha512(self, messages) -> np.ndarray:
        """RistrettoPoint::hash_from_bytes::<Sha512> of every message (a list of byte strings) on the GPU -> encodings [n][32]"""
        return self.hash_from_bytes_sha512_csr(*messages_csr(messages))

    def hash_from_bytes_sha512_csr(self, data, offsets) -> np.ndarray:
        """the same for a CSR batch held in numpy buffers: message i = data[offsets[i]:offsets[i + 1]]"""
        data, offsets = _csr_args(data, offsets)
        n = len(offsets) - 1
        out = np.zeros((n, 32), np.uint8)
        _check(self._lib.zkp_hash_from_bytes_sha512(self._h, n, _ptr(data), _ptr(offsets), _ptr(out)), "zkp_hash_from_bytes_sha512")
        return out

    # ---- Merlin operations on transcripts, batched (include/zkp_mi355x.h section 7) ----
    strobe_pos_after_append = staticmethod(strobe_pos_after_append)

    def transcripts_append_message(self, transcripts, label: bytes, data, offsets, shared_initial: bool = False) -> np.ndarray:
        """N x append_message(label, data[offsets[j]:offsets[j + 1]]) on the GPU.  transcripts: C-contiguous uint8 [N][208], advanced in
        place (shared_initial: row 0 is what every transcript starts from, all N rows are written).  Returns transcripts."""
        data, offsets = _csr_args(data, offsets)
        n = len(offsets) - 1
        ts = _blobs(transcripts, n)
        _check(self._lib.zkp_transcripts_append_message(self._h, n, int(bool(shared_initial)), _ptr(ts), bytes(label), _ptr(data), _ptr(offsets)),
               "zkp_transcripts_append_message")
        return ts

    def transcripts_challenge_bytes(self, transcripts, label: bytes, n_bytes: int) -> np.ndarray:
        """N x challenge_bytes(label, n_bytes) on the GPU -> uint8 [N][n_bytes]; transcripts (C-contiguous uint8 [N][208]) advance in place"""
        ts = _blobs(transcripts, len(transcripts))
        out = np.zeros((len(ts), n_bytes), np.uint8)
        _check(self._lib.zkp_transcripts_challenge_bytes(self._h, len(ts), _ptr(ts), bytes(label), n_bytes, _ptr(out)), "zkp_transcripts_challenge_bytes")
        return out

    def transcripts_witness_rng(self, transcripts, label: bytes, witnesses, entropy, mode: int, count: int) -> np.ndarray:
        """N x TranscriptRng on the GPU: rekey with witnesses[j][k] (uint8 [N][m][wlen]) under label, finalize with entropy[j] (uint8 [N][32]),
        then count scalars (mode ZKP_RNG_SCALARS -> uint8 [N][count][32]) or one fill_bytes(count) (ZKP_RNG_BYTES -> uint8 [N][count]).  The
        transcripts (C-contiguous uint8 [N][208]) are read, never written."""
        ts = _blobs(transcripts, len(transcripts))
        n = len(ts)
        wit = np.ascontiguousarray(witnesses, np.uint8)
        ent = np.ascontiguousarray(entropy, np.uint8)
        if wit.ndim != 3 or len(wit) != n or ent.shape != (n, 32):
            raise ValueError("witnesses must be uint8 [N][m][wlen] and entropy uint8 [N][32]")
        out = np.zeros((n, count, 32) if mode == ZKP_RNG_SCALARS else (n, count), np.uint8)
        _check(self._lib.zkp_transcripts_witness_rng(self._h, n, _ptr(ts), bytes(label), wit.shape[1], wit.shape[2], _ptr(wit), _ptr(ent), mode, count, _ptr(out)),
               "zkp_transcripts_witness_rng")
        return out

    def transcripts_challenge_scalars(self, transcripts, label: bytes) -> np.ndarray:
        """N x get_challenge(label) on the GPU -> canonical scalars uint8 [N][32]; transcripts (C-contiguous uint8 [N][208]) advance in place"""
        ts = _blobs(transcripts, len(transcripts))
        out = np.zeros((len(ts), 32), np.uint8)
        _check(self._lib.zkp_transcripts_challenge_scalars(self._h, len(ts), _ptr(ts), bytes(label), _ptr(out)), "zkp_transcripts_challenge_scalars")
        return out

    def transcripts_append_points(self, transcripts, kind: bytes, var_label: bytes, points, validate: bool = False) -> np.ndarray:
        """N x { append_message(kind, var_label); append_message(b"val", points[j]) } on the GPU, the transcripts advanced in place -> status
        uint8 [N]: 1 = validate and row j is the identity's encoding (32 zero bytes), whose transcript stays as it was"""
        ts = _blobs(transcripts, len(transcripts))
        pts = np.ascontiguousarray(points, np.uint8)
        if pts.shape != (len(ts), 32):
            raise ValueError("points must be uint8 [N][32]")
        status = np.zeros(len(ts), np.uint8)
        _check(self._lib.zkp_transcripts_append_points(self._h, len(ts), _ptr(ts), bytes(kind), bytes(var_label), _ptr(pts), int(bool(validate)), _ptr(status)),
               "zkp_transcripts_append_points")
        return status

    # ---- scalars mod l, batched (include/zkp_mi355x.h section 6): [n][32] canonical scalars out ----
    def scalar_invert(self, s) -> np.ndarray:
        """Scalar::invert of every row (any 32 bytes, read mod l; 0 -> 0)"""
        s = _u8(s, 32)
        out = np.zeros((len(s), 32), np.uint8)
        _check(self._lib.zkp_sc_invert(self._h, len(s), _ptr(s), _ptr(out)), "zkp_sc_invert")
        return out

    def scalar_from_wide(self, wide) -> np.ndarray:
        """Scalar::from_bytes_mod_order_wide of every 64-byte row"""
        wide = _u8(wide, 64)
        out = np.zeros((len(wide), 32), np.uint8)
        _check(self._lib.zkp_sc_from_wide(self._h, len(wide), _ptr(wide), _ptr(out)), "zkp_sc_from_wide")
        return out

    def scalar_muladd(self, a, b, c=None) -> np.ndarray:
        """a * b + c mod l row by row; an operand of shape (32,) or (1, 32) is shared by all rows (stride 0); c = None: + 0"""
        n, (a, sa), (b, sb), (c, sc) = scalar_operands(a, b, c)
        out = np.zeros((n, 32), np.uint8)
        _check(self._lib.zkp_sc_muladd(self._h, n, _ptr(a), sa, _ptr(b), sb, _ptr(c), sc, _ptr(out)), "zkp_sc_muladd")
        return out

    def scalar_random(self, n: int, key: bytes, nonce: int = 0) -> np.ndarray:
        """n x Scalar::random drawn on the GPU: row i = from_bytes_mod_order_wide(ChaCha20 block i of (key, nonce))"""
        k = np.frombuffer(bytes(key), np.uint8).copy()
        if k.size != 32:
            raise ValueError("key must be 32 bytes")
        out = np.zeros((n, 32), np.uint8)
        _check(self._lib.zkp_sc_random(self._h, n, _ptr(k), nonce, _ptr(out)), "zkp_sc_random")
        return out

    def scalar_hash_from_bytes_sha512(self, messages) -> np.ndarray:
        """Scalar::hash_from_bytes::<Sha512> of every message (a list of byte strings) on the GPU"""
        return self.scalar_hash_from_bytes_sha512_csr(*messages_csr(messages))

    def scalar_hash_from_bytes_sha512_csr(self, data, offsets) -> np.ndarray:
        """the same for a CSR batch held in numpy buffers: message i = data[offsets[i]:offsets[i + 1]]"""
        data, offsets = _csr_args(data, offsets)
        n = len(offsets) - 1
        out = np.zeros((n, 32), np.uint8)
        _check(self._lib.zkp_sc_hash_from_bytes_sha512(self._h, n, _ptr(data), _ptr(offsets), _ptr(out)), "zkp_sc_hash_from_bytes_sha512")
        return out

    # ---- Scalar * basepoint, Scalar * point, batched (include/zkp_mi355x.h section 8): encodings [n][32] out ----
    def mul_base(self, scalars) -> np.ndarray:
        """scalars[i] * B for every row (any 32 bytes, read mod l), constant time -> encodings [n][32]"""
        s = _u8(scalars, 32)
        out = np.zeros((len(s), 32), np.uint8)
        _check(self._lib.zkp_mul_base(self._h, len(s), _ptr(s), _ptr(out)), "zkp_mul_base")
        return out

    def mul_points(self, scalars, points, flags: int = ZKP_CT) -> Tuple[np.ndarray, np.ndarray]:
        """scalars[i] * decode(points[i]) row by row -> (encodings [n][32], status [n]: 1 and a zero row where the point does not decode); an
        operand of shape (32,) or (1, 32) is shared by all rows (stride 0)"""
        n, (s, ss), (p, ps) = mul_operands(scalars, points)
        out = np.zeros((n, 32), np.uint8)
        status = np.zeros(n, np.uint8)
        _check(self._lib.zkp_mul_points(self._h, n, _ptr(s), ss, _ptr(p), ps, flags, _ptr(out), _ptr(status)), "zkp_mul_points")
        return out, status

    # ---- RistrettoPoint sums, batched (include/zkp_mi355x.h section 9): encodings out, status 1 and a zero row where an operand does not decode ----
    def add_points(self, a, b, op: int = ZKP_PT_ADD) -> Tuple[np.ndarray, np.ndarray]:
        """decode(a[i]) + decode(b[i]) (ZKP_PT_ADD) or - (ZKP_PT_SUB) row by row -> (encodings [n][32], status [n]); an operand of shape (32,) or
        (1, 32) is shared by all rows (stride 0)"""
        n, (a, sa), (b, sb) = mul_operands(a, b)
        out = np.zeros((n, 32), np.uint8)
        status = np.zeros(n, np.uint8)
        _check(self._lib.zkp_add_points(self._h, n, _ptr(a), sa, _ptr(b), sb, op, _ptr(out), _ptr(status)), "zkp_add_points")
        return out, status

    def sum_points(self, off, points, pidx=None, neg=None) -> Tuple[np.ndarray, np.ndarray]:
        """out[i] = encode(sum over t in [off[i], off[i + 1]) of +- decode(points[pidx[t]])) -> (out [n_sums][32], status [n_sums]); pidx = None:
        term t is point t; neg = None: every term is added, else neg[t] != 0 subtracts term t"""
        off, pidx, neg, points = sum_operands(off, points, pidx, neg)
        n_sums = len(off) - 1
        out = np.zeros((n_sums, 32), np.uint8)
        status = np.zeros(n_sums, np.uint8)
        _check(self._lib.zkp_sum_points(self._h, n_sums, _ptr(off), None if pidx is None else _ptr(pidx), None if neg is None else _ptr(neg), _ptr(points),
                                        len(points), _ptr(out), _ptr(status)), "zkp_sum_points")
        return out, status

    def msm_segments(self, off, scalars, points, pidx=None, flags: int = ZKP_VARTIME) -> Tuple[np.ndarray, np.ndarray]:
        """zkp_msm_segments: msm_many's results -- out[i] = encode(sum over t in [off[i], off[i + 1]) of scalars[t] * decode(points[pidx[t]])) ->
        (out [n_msm][32], status [n_msm]) -- with the term axis folded in levels, for segments of any length; pidx = None: term t uses point t"""
        off, pidx, _, points = sum_operands(off, points, pidx, None)
        n_msm, n_terms = len(off) - 1, int(off[-1])
        scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
        if len(scalars) != n_terms:
            raise ValueError("scalars length must equal off[-1]")
        out = np.zeros((n_msm, 32), np.uint8)
        status = np.zeros(n_msm, np.uint8)
        _check(self._lib.zkp_msm_segments(self._h, n_msm, _ptr(off), _ptr(scalars), None if pidx is None else _ptr(pidx), _ptr(points), len(points), flags,
                                          _ptr(out), _ptr(status)), "zkp_msm_segments")
        return out, status

    def msm_optional_many(self, off, scalars, points, pidx=None) -> Tuple[np.ndarray, np.ndarray]:
        """zkp_msm_optional_many: msm_many's variable-time results per segment -- out[i] = encode(sum over t in [off[i], off[i + 1]) of scalars[t] *
        decode(points[pidx[t]])) -> (out [n_seg][32], status [n_seg]) -- by the bucket method, many segments to a run; pidx = None: a point per term.
        VARIABLE TIME: public scalars only"""
        off, pidx, _, points = sum_operands(off, points, pidx, None)
        n_seg, n_terms = len(off) - 1, int(off[-1])
        scalars = _u8(scalars, 32) if n_terms else np.zeros((0, 32), np.uint8)
        if len(scalars) != n_terms:
            raise ValueError("scalars length must equal off[-1]")
        out = np.zeros((n_seg, 32), np.uint8)
        status = np.zeros(n_seg, np.uint8)
        _check(self._lib.zkp_msm_optional_many(self._h, n_seg, _ptr(off), _ptr(scalars), None if pidx is None else _ptr(pidx), _ptr(points), len(points),
                                               _ptr(out), _ptr(status)), "zkp_msm_optional_many")
        return out, status

    def scalar_reduce(self, op: int, off, a, aidx=None, b=None, bidx=None) -> np.ndarray:
        """zkp_sc_reduce: out[i] = the fold of the terms [off[i], off[i + 1]) -> [n_out][32] canonical scalars.  op = ZKP_SC_SUM (of a[ai(t)], empty: 0),
        ZKP_SC_PRODUCT (empty: 1) or ZKP_SC_DOT (of a[ai(t)] * b[bi(t)], empty: 0); ai(t) = aidx[t], or t with aidx = None (a then has off[-1] rows)"""
        off, a, aidx, b, bidx = reduce_operands(op, off, a, aidx, b, bidx)
        n_out = len(off) - 1
        out = np.zeros((n_out, 32), np.uint8)
        _check(self._lib.zkp_sc_reduce(self._h, op, n_out, _ptr(off), _ptr(a) if len(a) else None, len(a), _ptr(aidx),
                                       None if b is None or not len(b) else _ptr(b), 0 if b is None else len(b), _ptr(bidx), _ptr(out)), "zkp_sc_reduce")
        return out

    # ---- prefix sums and products over segments (include/zkp_mi355x.h section 13): one row per term ----
    def scalar_scan(self, op: int, off, a, aidx=None, exclusive: bool = False) -> np.ndarray:
        """zkp_sc_scan: out[t] = the fold of the terms of t's segment up to t (exclusive: before t; the identity at a segment's first term) ->
        [off[-1]][32] canonical scalars.  op = ZKP_SC_SUM or ZKP_SC_PRODUCT of a[ai(t)]; ai(t) = aidx[t], or t with aidx = None"""
        off, a, aidx, _, _ = reduce_operands(ZKP_SC_SUM, off, a, aidx)       # (shapes only: op is the library's to check)
        out = np.zeros((int(off[-1]), 32), np.uint8)
        _check(self._lib.zkp_sc_scan(self._h, op, int(bool(exclusive)), len(off) - 1, _ptr(off), _ptr(a) if len(a) else None, len(a), _ptr(aidx), _ptr(out)),
               "zkp_sc_scan")
        return out

    def point_scan(self, off, points, pidx=None, neg=None, exclusive: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """zkp_scan_points: out[t] = encode(the sum of +- decode(points[pidx[t']]) over the terms t' of t's segment up to t (exclusive: before t)) ->
        (out [off[-1]][32], status [off[-1]]); status 1 and a zero row where a point the row depends on does not decode; pidx = None: term t is point t"""
        off, pidx, neg, points = sum_operands(off, points, pidx, neg)
        n_terms = int(off[-1])
        out = np.zeros((n_terms, 32), np.uint8)
        status = np.zeros(n_terms, np.uint8)
        _check(self._lib.zkp_scan_points(self._h, int(bool(exclusive)), len(off) - 1, _ptr(off), None if pidx is None else _ptr(pidx),
                                         None if neg is None else _ptr(neg), _ptr(points) if len(points) else None, len(points), _ptr(out), _ptr(status)),
               "zkp_scan_points")
        return out, status

    # ---- bounded discrete logarithms to the basepoint (include/zkp_mi355x.h section 10): variable time by nature ----
    def prepare_dlog(self, baby_bits: int) -> None:
        """build (or replace) the context's baby-step table: the encodings of i B for i < 2**baby_bits, baby_bits in 4 .. 22"""
        _check(self._lib.zkp_ctx_prepare_dlog(self._h, baby_bits), "zkp_ctx_prepare_dlog")

    @property
    def dlog_baby_bits(self) -> int:
        """the size of the baby-step table the context holds; 0 = none yet"""
        return int(self._lib.zkp_dlog_baby_bits(self._h))

    def dlog_base(self, points, bits: int) -> Tuple[np.ndarray, np.ndarray]:
        """points [n][32] = encode(k B) -> (k uint64 [n], status uint8 [n]): status 0 = found (k < 2**bits), 1 = the encoding does not decode,
        2 = no k in range (k = 0 for both); bits in 1 .. 48.  A context without a table builds the default size first."""
        points = _u8(points, 32)
        n = len(points)
        out = np.zeros(n, np.uint64)
        status = np.zeros(n, np.uint8)
        _check(self._lib.zkp_dlog_base(self._h, n, _ptr(points), bits, _ptr(out), _ptr(status)), "zkp_dlog_base")
        return out, status

    # ---- ... to a base of the caller's, signed ranges: one table per slot, ZKP_DLOG_SLOTS slots per context ----
    def prepare_dlog_point(self, slot: int, base, baby_bits: int) -> None:
        """build (or replace) slot `slot` for the base with encoding `base` (32 bytes): the encodings of i G for i < 2**baby_bits, baby_bits in
        4 .. 22.  The same base and size again is a no-op."""
        base = _base32(base)
        _check(self._lib.zkp_ctx_prepare_dlog_point(self._h, slot, _ptr(base), baby_bits), "zkp_ctx_prepare_dlog_point")

    def release_dlog_point(self, slot: int) -> None:
        _check(self._lib.zkp_ctx_release_dlog_point(self._h, slot), "zkp_ctx_release_dlog_point")

    def dlog_point_slots(self):
        """[(base bytes or None, baby_bits)] for every slot; (None, 0) is an empty one"""
        out = []
        for slot in range(ZKP_DLOG_SLOTS):
            bb = int(self._lib.zkp_dlog_point_baby_bits(self._h, slot))
            base = np.zeros(32, np.uint8)
            if bb:
                _check(self._lib.zkp_dlog_point_base(self._h, slot, _ptr(base)), "zkp_dlog_point_base")
            out.append((base.tobytes() if bb else None, bb))
        return out

    def dlog_point(self, slot: int, points, bits: int, signed: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """points [n][32] = encode(k G), G the slot's base -> (k [n], status uint8 [n]) as dlog_base; signed: k in [-2**(bits - 1), 2**(bits - 1))
        as np.int64, else k < 2**bits as np.uint64"""
        points = _u8(points, 32)
        n = len(points)
        out = np.zeros(n, np.uint64)
        status = np.zeros(n, np.uint8)
        _check(self._lib.zkp_dlog_point(self._h, slot, n, _ptr(points), bits, ZKP_DLOG_SIGNED if signed else 0, _ptr(out), _ptr(status)), "zkp_dlog_point")
        return (out.view(np.int64) if signed else out), status

    def debug_sha512(self, data, offsets) -> np.ndarray:
        """the SHA-512 stage alone (test-hook build): CSR batch -> digests [n][64]"""
        self._need_hooks("zkp_debug_sha512")
        data, offsets = _csr_args(data, offsets)
        n = len(offsets) - 1
        out = np.zeros((n, 64), np.uint8)
        _check(self._lib.zkp_debug_sha512(self._h, n, _ptr(data), _ptr(offsets), _ptr(out)), "zkp_debug_sha512")
        return out

    def debug_quad_selftest(self, pairs) -> np.ndarray:
        pairs = _u8(pairs, 64)
        out = np.zeros((len(pairs), 4, 32), np.uint8)
        self._need_hooks("zkp_debug_quad_selftest")
        _check(self._lib.zkp_debug_quad_selftest(self._h, len(pairs), _ptr(pairs), _ptr(out)), "zkp_debug_quad_selftest")
        return out

    def debug_row_selftest(self, pairs) -> np.ndarray:
        """(test-hook build) one-limb-per-lane point arithmetic (csrc/rowfe.h): [n][64] encodings (P, Q) -> [n][3][32] = enc(2P), enc(P+Q), enc(2^11 P + Q)"""
        pairs = _u8(pairs, 64)
        out = np.zeros((len(pairs), 3, 32), np.uint8)
        self._need_hooks("zkp_debug_row_selftest")
        _check(self._lib.zkp_debug_row_selftest(self._h, len(pairs), _ptr(pairs), _ptr(out)), "zkp_debug_row_selftest")
        return out

    def debug_wave_cycles(self, cap: int = 1 << 20):
        """(test-hook build, after set_option(ZKP_TESTOPT_WAVE_CYCLES, 1)) -> (class[n], cycles[n]) of the term kernel's wavefronts since the last read"""
        self._need_hooks("zkp_debug_wave_cycles")
        buf = np.zeros(cap, np.uint64)
        n = self._lib.zkp_debug_wave_cycles(self._h, _ptr(buf), cap)
        if n < 0:
            _check(n, "zkp_debug_wave_cycles")
        buf = buf[:n]
        buf = buf[buf != 0]
        return (buf >> np.uint64(56)).astype(np.int64), (buf & np.uint64((1 << 56) - 1)).astype(np.int64)

    def last_schedule(self) -> dict:
        """(test-hook build) {choice: value} of the size-driven choices the last call made (zkp_debug_last_schedule), e.g.
        {"batch_encode": 1, "enc_groups": 2}; choices the call did not make are absent"""
        self._need_hooks("zkp_debug_last_schedule")
        buf = ctypes.create_string_buffer(1024)
        n = self._lib.zkp_debug_last_schedule(self._h, buf, 1024)
        if n < 0:
            _check(n, "zkp_debug_last_schedule")
        return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split())}

    def debug_fill_workspace(self, min_bytes: int, word: int) -> None:
        """(test-hook build) grow the device workspace to at least min_bytes as any call would, set every 32-bit word of all of it to `word`
        and wait for the context's streams: what earlier calls may have left behind, in one call (zkp_debug_fill_workspace)"""
        self._need_hooks("zkp_debug_fill_workspace")
        _check(self._lib.zkp_debug_fill_workspace(self._h, min_bytes, word & 0xffffffff), "zkp_debug_fill_workspace")

    def debug_ws_bytes(self) -> int:
        """(test-hook build) the size of the device workspace as it stands (zkp_debug_ws_bytes)"""
        self._need_hooks("zkp_debug_ws_bytes")
        return int(self._lib.zkp_debug_ws_bytes(self._h))

    def debug_ws_count(self, needle) -> int:
        """(test-hook build) how often the bytes of `needle` occur in the device workspace as it stands, read back to the host
        (zkp_debug_ws_count); raises inside a capture"""
        self._need_hooks("zkp_debug_ws_count")
        buf = np.frombuffer(bytes(needle), np.uint8).copy()
        n = int(self._lib.zkp_debug_ws_count(self._h, _ptr(buf), len(buf)))
        if n >= 1 << 63:                                      # (size_t)ZKP_ERR_*
            raise ZkpError(f"zkp_debug_ws_count failed with code {n - (1 << 64)}: {self._lib.zkp_last_error().decode()}")
        return n

    def prepare_fixed_points(self, encodings) -> None:
        """Hint: these points (the statement's common / static points) will be referenced by many terms."""
        encodings = _u8(encodings, 32)
        _check(self._lib.zkp_ctx_prepare_fixed_points(self._h, len(encodings), _ptr(encodings)), "zkp_ctx_prepare_fixed_points")

    # ---- device-buffer entry points (raw device pointers, e.g. torch tensor .data_ptr()) ----
    def set_stream(self, hip_stream: int) -> None:
        _check(self._lib.zkp_ctx_set_stream(self._h, hip_stream), "zkp_ctx_set_stream")

    def synchronize(self) -> None:
        _check(self._lib.zkp_ctx_synchronize(self._h), "zkp_ctx_synchronize")

    def msm_many_dev(self, n_msm, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, flags, d_out, d_status) -> None:
        _check(self._lib.zkp_msm_many_dev(self._h, n_msm, d_off, d_scalars, d_pidx, d_points, n_points, n_terms,
                                          flags, d_out, d_status), "zkp_msm_many_dev")

    def msm_optional_dev(self, n, d_scalars, d_points, d_out, d_status) -> None:
        _check(self._lib.zkp_msm_optional_dev(self._h, n, d_scalars, d_points, d_out, d_status), "zkp_msm_optional_dev")

    def from_uniform_bytes_dev(self, n, d_in, d_out) -> None:
        """zkp_from_uniform_bytes_dev: d_in [n][64] -> d_out [n][32], device pointers (16-byte aligned), queued on the context's stream"""
        _check(self._lib.zkp_from_uniform_bytes_dev(self._h, n, d_in, d_out), "zkp_from_uniform_bytes_dev")

    def hash_from_bytes_sha512_dev(self, n, d_msgs, msgs_len, d_offsets, d_out) -> None:
        """zkp_hash_from_bytes_sha512_dev: message i = d_msgs[d_offsets[i], d_offsets[i + 1]) (u64 offsets, 8-byte aligned) -> d_out [n][32]
        (16-byte aligned), device pointers, queued on the context's stream"""
        _check(self._lib.zkp_hash_from_bytes_sha512_dev(self._h, n, d_msgs, msgs_len, d_offsets, d_out), "zkp_hash_from_bytes_sha512_dev")

    def scalar_invert_dev(self, n, d_in, d_out) -> None:
        """zkp_sc_invert_dev: d_in [n][32] -> d_out [n][32] (may be d_in), device pointers (16-byte aligned), queued on the context's stream"""
        _check(self._lib.zkp_sc_invert_dev(self._h, n, d_in, d_out), "zkp_sc_invert_dev")

    def scalar_from_wide_dev(self, n, d_in, d_out) -> None:
        """zkp_sc_from_wide_dev: d_in [n][64] -> d_out [n][32]"""
        _check(self._lib.zkp_sc_from_wide_dev(self._h, n, d_in, d_out), "zkp_sc_from_wide_dev")

    def scalar_muladd_dev(self, n, d_a, a_stride, d_b, b_stride, d_c, c_stride, d_out) -> None:
        """zkp_sc_muladd_dev: strides 0 or 1 in elements, d_c = None: + 0"""
        _check(self._lib.zkp_sc_muladd_dev(self._h, n, d_a, a_stride, d_b, b_stride, d_c, c_stride, d_out), "zkp_sc_muladd_dev")

    def scalar_random_dev(self, n, key: bytes, nonce, d_out) -> None:
        """zkp_sc_random_dev: key = 32 host bytes; d_out [n][32]"""
        k = np.frombuffer(bytes(key), np.uint8).copy()
        if k.size != 32:
            raise ValueError("key must be 32 bytes")
        _check(self._lib.zkp_sc_random_dev(self._h, n, _ptr(k), nonce, d_out), "zkp_sc_random_dev")

    def scalar_hash_from_bytes_sha512_dev(self, n, d_msgs, msgs_len, d_offsets, d_out) -> None:
        """zkp_sc_hash_from_bytes_sha512_dev: arguments as hash_from_bytes_sha512_dev -> d_out [n][32] scalars"""
        _check(self._lib.zkp_sc_hash_from_bytes_sha512_dev(self._h, n, d_msgs, msgs_len, d_offsets, d_out), "zkp_sc_hash_from_bytes_sha512_dev")

    def mul_base_dev(self, n, d_scalars, d_out) -> None:
        """zkp_mul_base_dev: d_scalars [n][32] -> d_out [n][32], device pointers (16-byte aligned), queued on the context's stream"""
        _check(self._lib.zkp_mul_base_dev(self._h, n, d_scalars, d_out), "zkp_mul_base_dev")

    def mul_points_dev(self, n, d_scalars, s_stride, d_points, p_stride, flags, d_out, d_status) -> None:
        """zkp_mul_points_dev: strides 0 or 1 in elements; d_out [n][32] (may be d_points when p_stride = 1), d_status [n] bytes"""
        _check(self._lib.zkp_mul_points_dev(self._h, n, d_scalars, s_stride, d_points, p_stride, flags, d_out, d_status), "zkp_mul_points_dev")

    def add_points_dev(self, n, d_a, a_stride, d_b, b_stride, op, d_out, d_status) -> None:
        """zkp_add_points_dev: strides 0 or 1 in elements; d_out [n][32] (may be an operand of stride 1), d_status [n] bytes"""
        _check(self._lib.zkp_add_points_dev(self._h, n, d_a, a_stride, d_b, b_stride, op, d_out, d_status), "zkp_add_points_dev")

    def sum_points_dev(self, n_sums, d_off, d_pidx, d_neg, d_points, n_points, n_terms, d_out, d_status) -> None:
        """zkp_sum_points_dev: d_off u32 [n_sums + 1], d_pidx u32 [n_terms] or None, d_neg u8 [n_terms] or None, d_points [n_points][32] ->
        d_out [n_sums][32], d_status [n_sums]; nothing is read on the host, the launches depend on n_terms and n_sums alone"""
        _check(self._lib.zkp_sum_points_dev(self._h, n_sums, d_off, d_pidx, d_neg, d_points, n_points, n_terms, d_out, d_status), "zkp_sum_points_dev")

    def msm_segments_dev(self, n_msm, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, flags, d_out, d_status) -> None:
        """zkp_msm_segments_dev: d_off u32 [n_msm + 1], d_scalars [n_terms][32], d_pidx u32 [n_terms] or None, d_points [n_points][32] ->
        d_out [n_msm][32], d_status [n_msm] bytes; nothing is read on the host, the launches depend on n_terms and n_msm alone"""
        _check(self._lib.zkp_msm_segments_dev(self._h, n_msm, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, flags, d_out, d_status),
               "zkp_msm_segments_dev")

    def msm_optional_many_dev(self, n_seg, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, max_seg, d_out, d_status) -> None:
        """zkp_msm_optional_many_dev: d_off u32 [n_seg + 1], d_scalars [n_terms][32], d_pidx u32 [n_terms] or None, d_points [n_points][32] ->
        d_out [n_seg][32], d_status [n_seg] bytes; nothing is read on the host: one class, every segment padded to max_seg, the caller's promise that
        no segment is longer; n_terms must be d_off[n_seg]"""
        _check(self._lib.zkp_msm_optional_many_dev(self._h, n_seg, d_off, d_scalars, d_pidx, d_points, n_points, n_terms, max_seg, d_out, d_status),
               "zkp_msm_optional_many_dev")

    def scalar_reduce_dev(self, op, n_out, d_off, d_a, n_a, d_aidx, d_b, n_b, d_bidx, n_terms, d_out) -> None:
        """zkp_sc_reduce_dev: d_off u32 [n_out + 1], d_a [n_a][32], d_aidx u32 [n_terms] or None, d_b [n_b][32] / d_bidx (ZKP_SC_DOT, else None, 0,
        None) -> d_out [n_out][32]; nothing is read on the host, the launches depend on n_terms and n_out alone; n_terms must be d_off[n_out]"""
        _check(self._lib.zkp_sc_reduce_dev(self._h, op, n_out, d_off, d_a, n_a, d_aidx, d_b, n_b, d_bidx, n_terms, d_out), "zkp_sc_reduce_dev")

    def scalar_scan_dev(self, op, mode, n_seg, d_off, d_a, n_a, d_aidx, n_terms, d_out) -> None:
        """zkp_sc_scan_dev: d_off u32 [n_seg + 1], d_a [n_a][32], d_aidx u32 [n_terms] or None -> d_out [n_terms][32]; nothing is read on the host, the
        launches depend on n_terms alone; n_terms must be d_off[n_seg]"""
        _check(self._lib.zkp_sc_scan_dev(self._h, op, mode, n_seg, d_off, d_a, n_a, d_aidx, n_terms, d_out), "zkp_sc_scan_dev")

    def point_scan_dev(self, mode, n_seg, d_off, d_pidx, d_neg, d_points, n_points, n_terms, d_out, d_status) -> None:
        """zkp_scan_points_dev: d_off u32 [n_seg + 1], d_pidx u32 [n_terms] or None, d_neg u8 [n_terms] or None, d_points [n_points][32] ->
        d_out [n_terms][32], d_status [n_terms] bytes; nothing is read on the host, the launches depend on n_terms alone"""
        _check(self._lib.zkp_scan_points_dev(self._h, mode, n_seg, d_off, d_pidx, d_neg, d_points, n_points, n_terms, d_out, d_status), "zkp_scan_points_dev")

    def dlog_base_dev(self, n, d_points, bits, d_out, d_status) -> None:
        """zkp_dlog_base_dev: d_points [n][32] (16-byte aligned) -> d_out u64 [n], d_status u8 [n]; queued on the context's stream"""
        _check(self._lib.zkp_dlog_base_dev(self._h, n, d_points, bits, d_out, d_status), "zkp_dlog_base_dev")

    def dlog_point_dev(self, slot, n, d_points, bits, d_out, d_status, signed: bool = False) -> None:
        """zkp_dlog_point_dev: as dlog_base_dev over the slot's base; signed: d_out holds int64"""
        _check(self._lib.zkp_dlog_point_dev(self._h, slot, n, d_points, bits, ZKP_DLOG_SIGNED if signed else 0, d_out, d_status), "zkp_dlog_point_dev")

    def transcripts_append_message_dev(self, n, shared_initial, d_ts_in, d_ts_out, label: bytes, d_msgs, msgs_len, d_offsets) -> None:
        """zkp_transcripts_append_message_dev: blobs 16-byte aligned (d_ts_out may be d_ts_in when not shared), d_offsets u64 [n + 1] 8-byte
        aligned, d_msgs of any alignment; every range is clamped to [0, msgs_len); queued on the context's stream"""
        _check(self._lib.zkp_transcripts_append_message_dev(self._h, n, int(bool(shared_initial)), d_ts_in, d_ts_out, bytes(label), d_msgs, msgs_len, d_offsets),
               "zkp_transcripts_append_message_dev")

    def transcripts_challenge_bytes_dev(self, n, d_ts, label: bytes, n_bytes, d_out) -> None:
        """zkp_transcripts_challenge_bytes_dev: d_ts [n][208] (16-byte aligned) advanced in place, d_out [n][n_bytes]"""
        _check(self._lib.zkp_transcripts_challenge_bytes_dev(self._h, n, d_ts, bytes(label), n_bytes, d_out), "zkp_transcripts_challenge_bytes_dev")

    def transcripts_witness_rng_dev(self, n, d_ts, label: bytes, m, wlen, d_witnesses, d_entropy, mode, count, d_out) -> None:
        """zkp_transcripts_witness_rng_dev: d_ts [n][208] (16-byte aligned) is only read; d_witnesses [n][m][wlen], d_entropy [n][32];
        d_out [n][count][32] (ZKP_RNG_SCALARS) or [n][count] (ZKP_RNG_BYTES)"""
        _check(self._lib.zkp_transcripts_witness_rng_dev(self._h, n, d_ts, bytes(label), m, wlen, d_witnesses, d_entropy, mode, count, d_out),
               "zkp_transcripts_witness_rng_dev")

    def transcripts_challenge_scalars_dev(self, n, d_ts, label: bytes, d_out) -> None:
        """zkp_transcripts_challenge_scalars_dev: d_ts [n][208] (16-byte aligned) advanced in place, d_out [n][32]"""
        _check(self._lib.zkp_transcripts_challenge_scalars_dev(self._h, n, d_ts, bytes(label), d_out), "zkp_transcripts_challenge_scalars_dev")

    def transcripts_append_points_dev(self, n, d_ts, kind: bytes, var_label: bytes, d_points, validate, d_status) -> None:
        """zkp_transcripts_append_points_dev: d_ts [n][208] (16-byte aligned) advanced in place, d_points [n][32], d_status [n] (may be
        None / 0 when validate is false)"""
        _check(self._lib.zkp_transcripts_append_points_dev(self._h, n, d_ts, bytes(kind), bytes(var_label), d_points, int(bool(validate)), d_status),
               "zkp_transcripts_append_points_dev")

    # ---- batched 1-of-k OR-proofs (include/zkp_or_mi355x.h) ----------------------------------------------
    def or_prove(self, fst: "FusedStatement", transcripts, secrets, real, inst, common, entropy):
        """N disjunctions of k instances of the statement, proved on the GPU: transcripts C-contiguous uint8 [N][208] (advanced in place),
        secrets [N][m][32], real [N] (the branch each witness satisfies), inst [k][ni][N][32], common [ns][32], entropy [N][32]
        -> (challenges [N][k][32], responses [N][k][m][32], status [N]: 1 = a point of that proof did not decode)"""
        ts = _blobs(transcripts, len(transcripts))
        n, m = len(ts), fst.c.shape.n_secrets
        inst = np.ascontiguousarray(inst, np.uint8)
        k = or_branches(fst, inst, n)
        sec = np.ascontiguousarray(secrets, np.uint8).reshape(n, m, 32)
        rl = np.ascontiguousarray(real, np.uint8).reshape(n)
        com = np.ascontiguousarray(common, np.uint8).reshape(fst.n_static, 32)
        ent = np.ascontiguousarray(entropy, np.uint8).reshape(n, 32)
        chal, resp, status = np.zeros((n, k, 32), np.uint8), np.zeros((n, k, m, 32), np.uint8), np.zeros(n, np.uint8)
        _check(self._lib.zkp_or_prove(self._h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(sec), _ptr(rl), _ptr(inst), _ptr(com), _ptr(ent), _ptr(chal), _ptr(resp),
                                      _ptr(status)), "zkp_or_prove")
        return chal, resp, status

    def or_verify(self, fst: "FusedStatement", transcripts, inst, common, challenges, responses) -> np.ndarray:
        """The verifier of or_prove's proofs -> results uint8 [N]: 0 = accepted, 1 = rejected; transcripts advance in place"""
        ts = _blobs(transcripts, len(transcripts))
        n, m = len(ts), fst.c.shape.n_secrets
        inst = np.ascontiguousarray(inst, np.uint8)
        k = or_branches(fst, inst, n)
        com = np.ascontiguousarray(common, np.uint8).reshape(fst.n_static, 32)
        chal = np.ascontiguousarray(challenges, np.uint8).reshape(n, k, 32)
        resp = np.ascontiguousarray(responses, np.uint8).reshape(n, k, m, 32)
        res = np.ones(n, np.uint8)
        _check(self._lib.zkp_or_verify(self._h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(inst), _ptr(com), _ptr(chal), _ptr(resp), _ptr(res)), "zkp_or_verify")
        return res

    def or_prove_dev(self, fst: "FusedStatement", k, n, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_chal, d_resp, d_status) -> None:
        """zkp_or_prove_dev: device pointers (16-byte aligned where they hold 32-byte rows or transcripts), queued on the context's stream"""
        _check(self._lib.zkp_or_prove_dev(self._h, ctypes.byref(fst.c), k, n, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_chal, d_resp, d_status),
               "zkp_or_prove_dev")

    def or_verify_dev(self, fst: "FusedStatement", k, n, d_ts, d_inst, d_common, d_chal, d_resp, d_results) -> None:
        """zkp_or_verify_dev: as or_prove_dev; d_results [n] bytes, 0 = accepted"""
        _check(self._lib.zkp_or_verify_dev(self._h, ctypes.byref(fst.c), k, n, d_ts, d_inst, d_common, d_chal, d_resp, d_results), "zkp_or_verify_dev")

    # ---- batchable 1-of-k OR-proofs (include/zkp_or_batch_mi355x.h) --------------------------------------
    def or_prove_batchable(self, fst: "FusedStatement", transcripts, secrets, real, inst, common, entropy):
        """or_prove plus the commitments the prover hashed -> (commitments [N][k][nc][32], challenges, responses, status)"""
        ts = _blobs(transcripts, len(transcripts))
        n, m, nc = len(ts), fst.c.shape.n_secrets, fst.c.shape.n_constraints
        inst = np.ascontiguousarray(inst, np.uint8)
        k = or_branches(fst, inst, n)
        sec = np.ascontiguousarray(secrets, np.uint8).reshape(n, m, 32)
        rl = np.ascontiguousarray(real, np.uint8).reshape(n)
        com = np.ascontiguousarray(common, np.uint8).reshape(fst.n_static, 32)
        ent = np.ascontiguousarray(entropy, np.uint8).reshape(n, 32)
        coms, chal = np.zeros((n, k, nc, 32), np.uint8), np.zeros((n, k, 32), np.uint8)
        resp, status = np.zeros((n, k, m, 32), np.uint8), np.zeros(n, np.uint8)
        _check(self._lib.zkp_or_prove_batchable(self._h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(sec), _ptr(rl), _ptr(inst), _ptr(com), _ptr(ent), _ptr(coms),
                                                _ptr(chal), _ptr(resp), _ptr(status)), "zkp_or_prove_batchable")
        return coms, chal, resp, status

    def _or_batchable_args(self, fst, transcripts, inst, common, commitments, challenges, responses):
        ts = _blobs(transcripts, len(transcripts))
        n, m, nc = len(ts), fst.c.shape.n_secrets, fst.c.shape.n_constraints
        inst = np.ascontiguousarray(inst, np.uint8)
        k = or_branches(fst, inst, n)
        com = np.ascontiguousarray(common, np.uint8).reshape(fst.n_static, 32)
        coms = np.ascontiguousarray(commitments, np.uint8).reshape(n, k, nc, 32)
        chal = np.ascontiguousarray(challenges, np.uint8).reshape(n, k, 32)
        resp = np.ascontiguousarray(responses, np.uint8).reshape(n, k, m, 32)
        return ts, n, k, inst, com, coms, chal, resp

    def or_verify_batchable(self, fst: "FusedStatement", transcripts, inst, common, commitments, challenges, responses) -> np.ndarray:
        """The exact per-proof verifier of the batchable form -> results uint8 [N]: 0 = accepted; transcripts advance in place"""
        ts, n, k, inst, com, coms, chal, resp = self._or_batchable_args(fst, transcripts, inst, common, commitments, challenges, responses)
        res = np.ones(n, np.uint8)
        _check(self._lib.zkp_or_verify_batchable(self._h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(inst), _ptr(com), _ptr(coms), _ptr(chal), _ptr(resp), _ptr(res)),
               "zkp_or_verify_batchable")
        return res

    def or_batch_verify(self, fst: "FusedStatement", transcripts, inst, common, commitments, challenges, responses, weights16, debug: bool = False):
        """One verdict for N batchable proofs with one multiscalar sum of ns + N k (ni + nc) operands; weights16 uint8 [N][k][nc][16]
        -> verdict (0 = every proof verifies), or (verdict, coefficient vector [ns + N k (ni + nc)][32]) with debug"""
        ts, n, k, inst, com, coms, chal, resp = self._or_batchable_args(fst, transcripts, inst, common, commitments, challenges, responses)
        nc = fst.c.shape.n_constraints
        w = np.ascontiguousarray(weights16, np.uint8).reshape(n, k, nc, 16)
        verdict = ctypes.c_int(1)
        dbg = np.zeros((fst.n_static + n * k * (fst.c.shape.n_instance + nc), 32), np.uint8) if debug else None
        _check(self._lib.zkp_or_batch_verify(self._h, ctypes.byref(fst.c), k, n, _ptr(ts), _ptr(inst), _ptr(com), _ptr(coms), _ptr(chal), _ptr(resp), _ptr(w),
                                             ctypes.byref(verdict), None if dbg is None else _ptr(dbg)), "zkp_or_batch_verify")
        return (verdict.value, dbg) if debug else verdict.value

    def or_prove_batchable_dev(self, fst: "FusedStatement", k, n, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_coms, d_chal, d_resp, d_status) -> None:
        """zkp_or_prove_batchable_dev: as or_prove_dev, plus d_coms [n][k][nc][32]"""
        _check(self._lib.zkp_or_prove_batchable_dev(self._h, ctypes.byref(fst.c), k, n, d_ts, d_secrets, d_real, d_inst, d_common, d_entropy, d_coms, d_chal, d_resp,
                                                    d_status), "zkp_or_prove_batchable_dev")

    def or_verify_batchable_dev(self, fst: "FusedStatement", k, n, d_ts, d_inst, d_common, d_coms, d_chal, d_resp, d_results) -> None:
        """zkp_or_verify_batchable_dev: d_results [n] bytes, 0 = accepted"""
        _check(self._lib.zkp_or_verify_batchable_dev(self._h, ctypes.byref(fst.c), k, n, d_ts, d_inst, d_common, d_coms, d_chal, d_resp, d_results),
               "zkp_or_verify_batchable_dev")

    def or_batch_verify_dev(self, fst: "FusedStatement", k, n, d_ts, d_inst, d_common, d_coms, d_chal, d_resp, d_weights16, d_verdict) -> None:
        """zkp_or_batch_verify_dev: d_weights16 [n][k][nc][16]; d_verdict one uint32 word written on the context's stream, 0 = every proof verifies"""
        _check(self._lib.zkp_or_batch_verify_dev(self._h, ctypes.byref(fst.c), k, n, d_ts, d_inst, d_common, d_coms, d_chal, d_resp, d_weights16, d_verdict),
               "zkp_or_batch_verify_dev")

    # ---- fused statement flows on device-resident buffers (include/zkp_mi355x.h section 2c) -------------
    def fused_prove_dev(self, fst: "FusedStatement", n, strobe_pos, d_ts, d_secrets, d_table, d_entropy, d_chal, d_resp, d_coms, d_status) -> None:
        _check(self._lib.zkp_fused_prove_dev(self._h, ctypes.byref(fst.c), n, strobe_pos, d_ts, d_secrets, d_table, d_entropy, d_chal, d_resp, d_coms,
                                             d_status), "zkp_fused_prove_dev")

    def fused_verify_batchable_dev(self, fst: "FusedStatement", n, strobe_pos, d_ts, d_table, d_resp, d_w, d_results) -> None:
        """d_table = common || instance rows || commitments [n][nc]; d_w [n][nc][16]; d_results [n] bytes (0 = verified)"""
        _check(self._lib.zkp_fused_verify_batchable_dev(self._h, ctypes.byref(fst.c), n, strobe_pos, d_ts, d_table, d_resp, d_w, d_results),
               "zkp_fused_verify_batchable_dev")

    def fused_verify_compact_dev(self, fst: "FusedStatement", n, strobe_pos, d_ts, d_table, d_chal, d_resp, d_results) -> None:
        _check(self._lib.zkp_fused_verify_compact_dev(self._h, ctypes.byref(fst.c), n, strobe_pos, d_ts, d_table, d_chal, d_resp, d_results),
               "zkp_fused_verify_compact_dev")

    def fused_batch_verify_dev(self, fst: "FusedStatement", n, strobe_pos, d_ts, d_points, d_coms, d_resp, d_w, d_out, d_status) -> None:
        _check(self._lib.zkp_fused_batch_verify_dev(self._h, ctypes.byref(fst.c), n, strobe_pos, d_ts, d_points, d_coms, d_resp, d_w, d_out, d_status),
               "zkp_fused_batch_verify_dev")

    def fused_batch_verify_many_dev(self, fst: "FusedStatement", n_batches, n_each, strobe_pos, d_ts, d_points, d_coms, d_resp, d_w, d_out, d_status) -> None:
        """K batch verifications of n_each proofs in one pass; d_out [K][32], d_status [K][2] int32 (zkp_fused_batch_verify_many_dev)."""
        _check(self._lib.zkp_fused_batch_verify_many_dev(self._h, ctypes.byref(fst.c), n_batches, n_each, strobe_pos, d_ts, d_points, d_coms, d_resp, d_w,
                                                         d_out, d_status), "zkp_fused_batch_verify_many_dev")

    def fused_batch_verify_many(self, fst: "FusedStatement", n_batches: int, transcripts, inst, common, commitments, responses, weights16, want_coeffs: bool = False):
        """zkp_fused_batch_verify_many on host arrays: the len(transcripts) = n_batches * N_each proofs lie next to each other, batch b =
        proofs [b N_each, (b + 1) N_each) -> verdicts[n_batches] (0 = the batch verifies) [, the coefficient vector the device built];
        the transcripts [N][208] are advanced in place."""
        n = len(transcripts)
        if n_batches <= 0 or n % n_batches:
            raise ValueError("the number of proofs must be a multiple of n_batches")
        n_each = n // n_batches
        k = n_batches * fst.n_static + (fst.n_instance + len(fst._lhs)) * n
        verdicts = (ctypes.c_int * n_batches)(*([1] * n_batches))
        co = np.zeros((k, 32), np.uint8) if want_coeffs else None
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in (transcripts, inst, common, commitments, responses, weights16)]
        if arrs[1].shape != (fst.n_instance, n, 32) or arrs[2].shape != (fst.n_static, 32) or arrs[3].shape != (n, len(fst._lhs), 32) or \
                arrs[4].shape[:1] != (n,) or arrs[5].shape != (len(fst._lhs), n, 16) or arrs[0].shape != (n, 208):
            raise ValueError("array shapes do not match the statement / batch sizes")
        _check(self._lib.zkp_fused_batch_verify_many(self._h, ctypes.byref(fst.c), n_batches, n_each, *map(_ptr, arrs), verdicts, _ptr(co)),
               "zkp_fused_batch_verify_many")
        transcripts[...] = arrs[0]
        v = np.array(list(verdicts), np.int32)
        return (v, co) if want_coeffs else v

    # ---- ragged batches: transcripts at different STROBE positions (synchronous, host arrays; transcripts [N][208] advanced in place) ----
    @staticmethod
    def _ragged_call(transcripts, *args):
        ts = np.ascontiguousarray(transcripts, dtype=np.uint8)
        if ts.ndim != 2 or ts.shape[1] != 208:
            raise ValueError("transcripts must be [N][208] uint8")
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in args]
        return ts, arrs, [_ptr(a) for a in arrs]

    def fused_prove_ragged(self, fst: "FusedStatement", transcripts, secrets, inst, common, entropy=None, seed: Optional[bytes] = None):
        """zkp_fused_prove_ragged -> (challenges [N][32], responses [N][m][32], commitments [N][nc][32], invalid_point); entropy [N][32]
        or a 40-byte seed, exactly one."""
        n, m, nc = len(transcripts), fst.c.shape.n_secrets, len(fst._lhs)
        chal, resp, coms = np.zeros((n, 32), np.uint8), np.zeros((n, m, 32), np.uint8), np.zeros((n, nc, 32), np.uint8)
        sd = None if seed is None else np.frombuffer(bytes(seed), np.uint8).copy()
        ts, _, p = self._ragged_call(transcripts, secrets, inst, common, entropy, sd)
        inv = ctypes.c_int(1)
        _check(self._lib.zkp_fused_prove_ragged(self._h, ctypes.byref(fst.c), n, _ptr(ts), *p, _ptr(chal), _ptr(resp), _ptr(coms), ctypes.byref(inv)),
               "zkp_fused_prove_ragged")
        transcripts[...] = ts
        return chal, resp, coms, inv.value

    def fused_verify_compact_ragged(self, fst: "FusedStatement", transcripts, inst, common, challenges, responses) -> np.ndarray:
        """zkp_fused_verify_compact_ragged -> results [N] (0 = accepted)"""
        n = len(transcripts)
        res = np.ones(n, np.uint8)
        ts, _, p = self._ragged_call(transcripts, inst, common, challenges, responses)
        _check(self._lib.zkp_fused_verify_compact_ragged(self._h, ctypes.byref(fst.c), n, _ptr(ts), *p, _ptr(res)), "zkp_fused_verify_compact_ragged")
        transcripts[...] = ts
        return res

    def fused_verify_batchable_ragged(self, fst: "FusedStatement", transcripts, inst, common, commitments, responses, weights16) -> np.ndarray:
        """zkp_fused_verify_batchable_ragged -> results [N] (0 = accepted); weights16 [N][nc][16]"""
        n = len(transcripts)
        res = np.ones(n, np.uint8)
        ts, _, p = self._ragged_call(transcripts, inst, common, commitments, responses, weights16)
        _check(self._lib.zkp_fused_verify_batchable_ragged(self._h, ctypes.byref(fst.c), n, _ptr(ts), *p, _ptr(res)), "zkp_fused_verify_batchable_ragged")
        transcripts[...] = ts
        return res

    def fused_batch_verify_many_ragged(self, fst: "FusedStatement", n_batches: int, transcripts, inst, common, commitments, responses, weights16=None,
                                       seed: Optional[bytes] = None) -> np.ndarray:
        """zkp_fused_batch_verify_many_ragged -> verdicts [n_batches] (0 = the batch verifies); weights16 [nc][N][16] or a 40-byte seed"""
        n = len(transcripts)
        if n_batches <= 0 or n % n_batches:
            raise ValueError("the number of proofs must be a multiple of n_batches")
        verdicts = (ctypes.c_int * n_batches)(*([1] * n_batches))
        sd = None if seed is None else np.frombuffer(bytes(seed), np.uint8).copy()
        ts, _, p = self._ragged_call(transcripts, inst, common, commitments, responses, weights16, sd)
        _check(self._lib.zkp_fused_batch_verify_many_ragged(self._h, ctypes.byref(fst.c), n_batches, n // n_batches, _ptr(ts), *p, verdicts),
               "zkp_fused_batch_verify_many_ragged")
        transcripts[...] = ts
        return np.array(list(verdicts), np.int32)

    def fused_hash_to_group_ragged(self, transcripts, label: bytes = b"output") -> np.ndarray:
        """zkp_fused_hash_to_group_ragged -> encodings [N][32]; transcripts [N][208] advanced in place"""
        ts = np.ascontiguousarray(transcripts, dtype=np.uint8)
        out = np.zeros((len(ts), 32), np.uint8)
        _check(self._lib.zkp_fused_hash_to_group_ragged(self._h, len(ts), _ptr(ts), bytes(label), _ptr(out)), "zkp_fused_hash_to_group_ragged")
        transcripts[...] = ts
        return out

    def fused_verify_batchable_coeffs(self, fst: "FusedStatement", transcripts, inst, common, commitments, responses, weights16):
        """zkp_fused_verify_batchable_coeffs on host arrays -> (results[N], coefficient vectors [N][np + nc][32]); the
        transcripts [N][208] are advanced in place."""
        n = len(transcripts)
        k = fst.n_static + fst.n_instance + len(fst._lhs)
        res = np.ones(n, np.uint8)
        co = np.zeros((n, k, 32), np.uint8)
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in (transcripts, inst, common, commitments, responses, weights16)]
        _check(self._lib.zkp_fused_verify_batchable_coeffs(self._h, ctypes.byref(fst.c), n, *map(_ptr, arrs), _ptr(res), _ptr(co)),
               "zkp_fused_verify_batchable_coeffs")
        transcripts[...] = arrs[0]
        return res, co

    @property
    def ct_lookups(self):
        """the values of ZKP_OPT_CT_LOOKUP this build of the library has: (0,) = lane crossbar only (7-bit fixed-base windows, the shipped shape);
        (0, 1, 2) in a -DZKP_HOT_W=6 build (masked scans and the LDS rows of rounds 2 - 4 exist for the 6-bit window only)"""
        return (0, 1, 2) if "6-bit" in self.version else (0,)

    def set_option(self, option: int, value: int) -> None:
        """Tuning knobs of include/zkp_mi355x.h (ZKP_OPT_*); results never depend on them."""
        _check(self._lib.zkp_ctx_set_option(self._h, option, value), "zkp_ctx_set_option")

    def capture_begin(self) -> None:
        """Start recording what is enqueued on this context's stream into a HIP graph (zkp_ctx_capture_begin)."""
        _check(self._lib.zkp_ctx_capture_begin(self._h), "zkp_ctx_capture_begin")

    def capture_end(self) -> "Graph":
        g = ctypes.c_void_p()
        _check(self._lib.zkp_ctx_capture_end(self._h, ctypes.byref(g)), "zkp_ctx_capture_end")
        return Graph(self, g)

    def capture_abort(self) -> None:
        """End and discard a capture (after a failed call inside it); the context is usable again."""
        _check(self._lib.zkp_ctx_capture_abort(self._h), "zkp_ctx_capture_abort")

    def capture(self):
        """Context manager around capture_begin / capture_end: `with eng.capture() as cap: ...calls...` then `cap.graph`.  An
        exception inside the block aborts the capture (zkp_ctx_capture_abort) instead of leaving the stream in capture mode."""
        return _Capture(self)

    def set_profiling(self, enabled: bool) -> None:
        _check(self._lib.zkp_ctx_set_profiling(self._h, int(enabled)), "zkp_ctx_set_profiling")

    def last_timing(self):
        arr = (ctypes.c_float * len(K_NAMES))()
        tot = ctypes.c_float()
        rc = self._lib.zkp_ctx_last_timing(self._h, arr, ctypes.byref(tot))
        if rc < 0:
            _check(rc, "zkp_ctx_last_timing")
        return {k: float(arr[i]) for i, k in enumerate(K_NAMES)}, float(tot.value)

    def last_kernels(self):
        """{timing kind: [kernel names as rocprofv3 prints them]} for the kinds whose kernel variant the last call picked at run time"""
        out = {}
        buf = ctypes.create_string_buffer(512)
        for i, k in enumerate(K_NAMES):
            n = self._lib.zkp_ctx_last_kernels(self._h, i, buf, len(buf))
            if n >= len(buf):                                        # (a call of many runs names every one of them: zkp_msm_optional_many)
                buf = ctypes.create_string_buffer(n + 1)
                n = self._lib.zkp_ctx_last_kernels(self._h, i, buf, len(buf))
            if n > 0:
                out[k] = buf.value.decode().split(";")
        return out


def or_branches(fst: "FusedStatement", inst: np.ndarray, n: int) -> int:
    """k of an OR-proof call, read off inst [k][ni][N][32]"""
    if inst.ndim != 4 or inst.shape[1:] != (fst.n_instance, n, 32) or len(inst) == 0:
        raise ValueError("inst must be uint8 [k][%d][%d][32] with k >= 1" % (fst.n_instance, n))
    return len(inst)


class _Capture:
    def __init__(self, eng: "Engine"):
        self._eng, self.graph = eng, None

    def __enter__(self):
        self._eng.capture_begin()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            self._eng.capture_abort()
            return False
        self.graph = self._eng.capture_end()
        return False


class Graph:
    """zkp_graph: a recorded chain of *_dev calls, replayed with one host call.  launch() raises ZkpError ("stale graph") when
    the context's workspace or plans changed after the capture (see zkp_mi355x.h, HIP graphs: lifetime rules)."""

    def __init__(self, eng: "Engine", handle):
        self._eng, self._h = eng, handle

    def launch(self) -> None:
        _check(self._eng._lib.zkp_graph_launch(self._h, self._eng._h), "zkp_graph_launch")

    def close(self) -> None:
        if self._h:
            self._eng._lib.zkp_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BatchStatementC(ctypes.Structure):
    _fields_ = [("n_secrets", ctypes.c_uint32), ("n_static", ctypes.c_uint32), ("n_instance", ctypes.c_uint32),
                ("n_constraints", ctypes.c_uint32), ("cons_lhs", ctypes.c_void_p), ("cons_off", ctypes.c_void_p),
                ("cons_sc", ctypes.c_void_p), ("cons_pt", ctypes.c_void_p)]


class _FusedStatementC(ctypes.Structure):
    _fields_ = [("shape", _BatchStatementC), ("label", ctypes.c_char_p), ("secret_labels", ctypes.POINTER(ctypes.c_char_p)),
                ("point_labels", ctypes.POINTER(ctypes.c_char_p)), ("alloc_order", ctypes.c_void_p), ("alloc_seq", ctypes.c_void_p)]


class FusedStatement:
    """zkp_fused_statement (include/zkp_mi355x.h): the statement in point-id form (static ids first, then instance ids)
    with its transcript labels.  points = [(label, is_common)] in allocation order; constraints = [(lhs, [(secret, point)])]
    with indices into `secrets` / `points`, exactly as Prover/Verifier::constrain receives them.  alloc_seq (optional) =
    the caller's allocation calls in order, [("s", secret index) | ("p", point index)], when scalars and points are
    interleaved; default: every secret before the first point (define_proof!'s order)."""

    def __init__(self, proof_label: bytes, secrets, points, constraints, alloc_seq=None):
        ns = sum(1 for _, c in points if c)
        rank, k_c, k_i = [], 0, 0
        for _, c in points:
            if c:
                rank.append(k_c); k_c += 1
            else:
                rank.append(ns + k_i); k_i += 1
        self.n_static, self.n_instance = k_c, k_i
        self._lhs = np.array([rank[l] for l, _ in constraints], np.uint32)
        off, sc, pt = [0], [], []
        for _, lc in constraints:
            for s_, p_ in lc:
                sc.append(s_); pt.append(rank[p_])
            off.append(len(sc))
        self._off = np.array(off, np.uint32)
        self._sc = np.array(sc, np.uint32)
        self._pt = np.array(pt, np.uint32)
        self._order = np.array(rank, np.uint32)
        plabels = [None] * len(points)
        for (name, _), r in zip(points, rank):
            plabels[r] = bytes(name)
        self._sl = (ctypes.c_char_p * max(1, len(secrets)))(*[bytes(x) for x in secrets])
        self._pl = (ctypes.c_char_p * max(1, len(points)))(*plabels)
        self._label = bytes(proof_label)
        self.c = _FusedStatementC(_BatchStatementC(len(secrets), k_c, k_i, len(constraints), _ptr(self._lhs), _ptr(self._off), _ptr(self._sc), _ptr(self._pt)),
                                  self._label, self._sl, self._pl, _ptr(self._order), None)
        if alloc_seq is not None:
            self._seq = np.array([(0x80000000 | i) if kind == "s" else rank[i] for kind, i in alloc_seq], np.uint32)
            self.c.alloc_seq = _ptr(self._seq)

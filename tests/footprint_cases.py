"""(helper module of tests/test_gpu_footprint.py and tests/test_host_footprint.py)
The FOOTPRINT catalogue: for every call of the C ABI that writes through a pointer of the caller's, which rows of which operand it owns -- and
one check that a call wrote exactly those rows, with the expected bytes, and nothing else.

An entry is a Case: the function's name, its form ("dev": device pointers, "host": host pointers with a context, "batch": a *_batch call of
include/zkp_toolbox.h on the host backend, ctx == NULL) and a builder of its argument list.  A pointer argument is an Op:

    role        "in" | "out" | "inout"; an optional operand (in_optional / out_optional of the catalogue's table) is a case with the Op and a
                case with None in its place
    data        the rows the caller hands in, uint8 [rows][row bytes] (in, inout)
    expected    the rows the call must leave, uint8 [rows][row bytes] (out, inout; an `in` operand must be left as it was)
    align       device pointers: the alignment the header promises to accept -- 16, 8, 4 or 1 ("any"); host pointers get the natural
                alignment of their C type (`elem` bytes: a uint8 array starts at an odd address)

Expected bytes come from oracle.cbind (the C oracle), oracle.model and Python integers, over the operands of the existing case modules; nothing
here calls the code under test.  Every row-wise expectation is computed once at the largest size and cut down for the smaller ones.

run_case() puts every operand in the middle of a larger buffer -- guards of max(4096 bytes, 256 rows) on both sides, 256 being the largest
workgroup that stores to caller memory -- at the minimum alignment and no better, prefills all of it with 0x80 | ((37 i) & 0x7f) (no byte of which
is a status value), makes the call through the raw C ABI and compares the WHOLE buffer with the prefill in which the operand's rows are replaced
by the expected bytes.  A difference is reported as (row, byte within row) relative to the operand's start; negative rows are the front guard."""
import ctypes
import functools
import hashlib

import numpy as np

from oracle import cbind as C
from oracle import model as M
from tests import dlog_cases as DC
from tests import dlog_point_cases as DPC
from tests import point_mul_cases as PC
from tests import point_sum_cases as PS
from tests import scalar_reduce_cases as SR
from tests import scan_cases as SCN
from tests import transcript_ops_cases as TO
from tests import transcript_rng_cases as TR
from tests.scalar_edge_cases import L, VALUES, random_256

ROW_SIZES = (1, 63, 65, 257)            # one lane per row: a lone lane, a partial wavefront, a wavefront + 1, a 256-lane workgroup + 1
TRANSCRIPT_SIZES = (1, 33, 65, 257)     # one transcript wavefront carries 32 proofs
GUARD_BYTES, GUARD_ROWS = 4096, 256
SLACK = 1024                            # room for the alignment and the phase shift of a view
CTX = object()                          # stands for the context in an argument list
ZKP_CT, ZKP_VARTIME = 1, 0
DLOG_BABY_BITS, DLOG_BITS, DLOG_SLOT, DLOG_BASE = 8, 10, 0, "H"


# ---- operands and cases --------------------------------------------------------------------------------------------------------------------------
def _rows(a):
    """(uint8 [rows][row bytes], element size) of an array of any dtype: a 1-D array is one element per row"""
    a = np.ascontiguousarray(a)
    elem = a.dtype.itemsize
    width = elem if a.ndim == 1 else elem * int(np.prod(a.shape[1:]))
    return a.view(np.uint8).reshape(len(a), width).copy(), elem


class Op:
    def __init__(self, name, role, data=None, expected=None, align=16, elem=1):
        self.name, self.role, self.align, self.elem = name, role, align, elem
        self.data = data
        self.expected = data if role == "in" else expected
        assert self.expected is not None and self.expected.ndim == 2 and self.expected.dtype == np.uint8, name
        assert data is None or data.shape == self.expected.shape, name
        self.rows, self.row_bytes = self.expected.shape

    def __repr__(self):
        return "%s(%s [%d][%d] align %d)" % (self.name, self.role, self.rows, self.row_bytes, self.align)


def IN(name, arr, align=None):
    data, elem = _rows(arr)
    return Op(name, "in", data, align=align or (16 if data.shape[1] % 16 == 0 and data.shape[1] else elem), elem=elem)


def OUT(name, expected, align=None):
    exp, elem = _rows(expected)
    return Op(name, "out", None, exp, align=align or (16 if exp.shape[1] % 16 == 0 and exp.shape[1] else elem), elem=elem)


def INOUT(name, arr, expected, align=16):
    data, elem = _rows(arr)
    return Op(name, "inout", data, _rows(expected)[0], align=align, elem=elem)


class Case:
    """fn(*build()) is one call; setup(lib, ctx) prepares what the call needs (a table) and may return an undo(); finish names the call that
    completes an asynchronous job (zkp_ctx_job_wait), made with the context alone once fn has returned 0"""

    def __init__(self, fn, form, size, variant, build, setup=None, finish=None):
        self.fn, self.form, self.build, self.setup, self.finish = fn, form, build, setup, finish
        name = fn[4:] if fn.startswith("zkp_") else fn
        self.id = "-".join([name, str(size)] + ([variant] if variant else []))

    def __repr__(self):
        return self.id


CASES = []


def add(fn, form, size, variant, build, setup=None, finish=None):
    CASES.append(Case(fn, form, size, variant, build, setup, finish))


def cases(form):
    return [c for c in CASES if c.form == form]


def catalogued():
    return {c.fn for c in CASES}


# ---- the check -----------------------------------------------------------------------------------------------------------------------------------
def prefill(total):
    i = np.arange(total, dtype=np.int64)
    return (0x80 | ((37 * i) & 0x7f)).astype(np.uint8)


def guard_bytes(op):
    return max(GUARD_BYTES, GUARD_ROWS * op.row_bytes)


def view_start(addr, guard, align):
    """the first offset >= guard at which addr + offset is a multiple of align and of nothing larger (align 1: an odd address)"""
    start = guard
    while (addr + start) % align or (addr + start) % (2 * align) == 0:
        start += 1
    return start


class _HostBuffers:
    device = False

    def alloc(self, total):
        buf = np.zeros(total, np.uint8)
        return buf, buf.ctypes.data

    def store(self, buf, image):
        buf[:] = image

    def load(self, buf):
        return buf.copy()

    def ready(self):
        pass


class _DeviceBuffers:
    device = True

    def __init__(self, device=0):
        import torch
        self.torch, self.dev = torch, "cuda:%d" % device

    def alloc(self, total):
        buf = self.torch.empty(total, dtype=self.torch.uint8, device=self.dev)
        return buf, buf.data_ptr()

    def store(self, buf, image):
        buf.copy_(self.torch.from_numpy(image))

    def load(self, buf):
        return buf.cpu().numpy()

    def ready(self):
        self.torch.cuda.synchronize()            # the uploads ran on torch's stream, the call runs on the context's


def first_difference(op, start, got, want):
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    d = int(bad[0]) - start
    rb = max(op.row_bytes, 1)
    return "%s: first differing byte at (row %d, byte %d) of %d rows of %d bytes: got 0x%02x, want 0x%02x%s; %d bytes differ" % (
        op.name, d // rb, d % rb, op.rows, op.row_bytes, got[bad[0]], want[bad[0]],
        " (prefill)" if not 0 <= d < op.rows * op.row_bytes else "", len(bad))


def run_case(case, lib, ctx, device):
    """make the call of `case` on guarded buffers and return the list of failures (empty: the footprint is exact)"""
    mem = _DeviceBuffers() if device else _HostBuffers()
    args = case.build()
    placed = {}
    for a in args:
        if isinstance(a, Op) and id(a) not in placed:
            guard = guard_bytes(a)
            nbytes = a.rows * a.row_bytes
            align = a.align if device else a.elem
            buf, addr = mem.alloc(2 * guard + nbytes + SLACK)
            # every operand of a call starts a little later in its buffer than the one before it, so that the prefills of operands next to each
            # other in the argument list are out of phase (the prefill repeats after 128 bytes: operands 64 / align apart -- four at 16 bytes --
            # coincide again): guard bytes of an input that a copy carries into the guard of the output next to it do not pass for prefill
            start = view_start(addr, guard + 2 * align * (len(placed) % 16), align)
            image = prefill(2 * guard + nbytes + SLACK)
            want = image.copy()
            want[start:start + nbytes] = a.expected.reshape(-1)
            if a.data is not None:
                image[start:start + nbytes] = a.data.reshape(-1)
            mem.store(buf, image)
            placed[id(a)] = (a, buf, addr + start, start, want)
    mem.ready()
    undo = case.setup(lib, ctx) if case.setup else None
    try:
        argv = [ctx if a is CTX else ctypes.c_void_p(placed[id(a)][2]) if isinstance(a, Op) else a for a in args]
        rc = getattr(lib, case.fn)(*argv)
        if rc == 0 and case.finish:
            rc = getattr(lib, case.finish)(ctx)
        if device and ctx is not None:
            src = lib.zkp_ctx_synchronize(ctx)
            assert src == 0, "zkp_ctx_synchronize after %s: %d" % (case.fn, src)
    finally:
        if undo:
            undo()
    if rc != 0:
        return ["%s refused a valid job: rc = %d" % (case.fn, rc)]
    failures = []
    for a, buf, _, start, want in placed.values():
        msg = first_difference(a, start, mem.load(buf), want)
        if msg:
            failures.append(msg)
    return failures


# ---- references ----------------------------------------------------------------------------------------------------------------------------------
NMAX = max(ROW_SIZES)


def sc_rows(vals):
    return SR.rows([int(v) for v in vals])


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def status8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def oracle_products(scalars, points, flags=ZKP_CT):
    """(out [n][32], status [n]) of scalars[i] * points[i] from the C oracle"""
    n = len(scalars)
    C.build()
    return C.msm_many(np.arange(n + 1, dtype=np.uint32), scalars, np.arange(n, dtype=np.uint32), points, flags)


def oracle_pairs(a, b, op):
    """(out [n][32], status [n]) of a[i] +- b[i] from the C oracle: one two-term sum per row with the scalars 1 and +-1"""
    n = len(a)
    C.build()
    sc = np.tile(sc_rows([1, L - 1 if op else 1]), (n, 1))
    pts = np.ascontiguousarray(np.stack([a, b], axis=1).reshape(2 * n, 32))
    return C.msm_many(np.arange(0, 2 * n + 1, 2, dtype=np.uint32), sc, np.arange(2 * n, dtype=np.uint32), pts, 0)


def spread(a, stride, n, shared_row=3):
    """the operand rows of a strided argument: n rows (stride 1) or the one shared row (stride 0)"""
    a = PC.tiled(a, n)
    return a if stride else np.ascontiguousarray(a[shared_row % n:shared_row % n + 1])


def broadcast(a, n):
    return a if len(a) == n else np.repeat(a, n, axis=0)


@functools.lru_cache(maxsize=None)
def scalar_ints(seed, n=NMAX):
    """the catalogue of tests/scalar_edge_cases.py first, then seeded 256-bit integers"""
    return tuple((VALUES + random_256(seed, n))[:n])


def chacha20_block(key: bytes, counter: int, nonce: int) -> bytes:
    """RFC 8439 section 2.3 with a 64-bit counter (state words 12-13) and a 64-bit nonce (14-15), as include/zkp_toolbox.h lays them out"""
    def rotl(v, r):
        return ((v << r) | (v >> (32 - r))) & 0xffffffff
    st = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]
    st += [counter & 0xffffffff, counter >> 32, nonce & 0xffffffff, nonce >> 32]
    x = list(st)

    def quarter(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 7)
    for _ in range(10):
        quarter(0, 4, 8, 12); quarter(1, 5, 9, 13); quarter(2, 6, 10, 14); quarter(3, 7, 11, 15)
        quarter(0, 5, 10, 15); quarter(1, 6, 11, 12); quarter(2, 7, 8, 13); quarter(3, 4, 9, 14)
    return b"".join(((x[i] + st[i]) & 0xffffffff).to_bytes(4, "little") for i in range(16))


def csr_lens(n):
    """n segments of 40, 1 and 0 terms in turn, the last one empty"""
    return [(40, 1, 0)[i % 3] for i in range(n - 1)] + [0]


def messages(n):
    """n messages of 0, 33 and 167 bytes in turn as a CSR batch (data uint8, offsets uint64 [n + 1]); data is never empty"""
    msgs = [TO.message((0, 33, 167)[j % 3], j) for j in range(n)]
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return msgs, np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy(), off


# ---- (8) Scalar * basepoint, Scalar * point; (9) pairs -------------------------------------------------------------------------------------------
def _mul_base(form, n):
    s = PC.tiled(PC.base_operands(), n)
    exp = PC.tiled(PC.base_expected(), n)
    ops = [IN("scalars", s), OUT("out", exp)]
    if form == "batch":
        return lambda t: [None, n, ops[0], t, ops[1]]
    return [CTX, n] + ops


def _strided_pairs(kind, form, n, sa, sb, flag):
    """zkp_mul_points (kind "mul": a = scalars, b = points, flag = ZKP_CT / ZKP_VARTIME) and zkp_add_points (kind "add": flag = op)"""
    if kind == "mul":
        a0, b0, _ = PC.pair_operands()
    else:
        a0, b0, _ = PS.pair_operands()
    a, b = spread(a0, sa, n), spread(b0, sb, n, shared_row=0 if kind == "mul" else 1)
    if kind == "mul":
        out, st = oracle_products(broadcast(a, n), broadcast(b, n))
    else:
        out, st = oracle_pairs(broadcast(a, n), broadcast(b, n), flag)
    ops = [IN("a", a), IN("b", b), OUT("out", out), OUT("status", status8(st), align=1)]
    if form == "batch":
        return lambda t: [None, n, ops[0], sa, ops[1], sb, flag, t, ops[2], ops[3]]
    return [CTX, n, ops[0], sa, ops[1], sb, flag, ops[2], ops[3]]


for _n in ROW_SIZES:
    for _form, _fn in (("dev", "zkp_mul_base_dev"), ("host", "zkp_mul_base")):
        add(_fn, _form, _n, "", lambda f=_form, n=_n: _mul_base(f, n))
    for _t in (1, 3):
        add("zkp_basepoint_mul_batch", "batch", _n, "t%d" % _t, lambda n=_n, t=_t: _mul_base("batch", n)(t))
    for _sa, _sb in ((1, 1), (0, 1), (1, 0)):
        _v = "s%dp%d" % (_sa, _sb)
        for _form, _fn in (("dev", "zkp_mul_points_dev"), ("host", "zkp_mul_points")):
            for _flag, _fname in ((ZKP_CT, "ct"), (ZKP_VARTIME, "vartime")):
                add(_fn, _form, _n, _v + "-" + _fname, lambda f=_form, n=_n, sa=_sa, sb=_sb, fl=_flag: _strided_pairs("mul", f, n, sa, sb, fl))
        for _t in (1, 3):
            add("zkp_point_mul_batch", "batch", _n, "%s-t%d" % (_v, _t),
                lambda n=_n, sa=_sa, sb=_sb, t=_t: _strided_pairs("mul", "batch", n, sa, sb, ZKP_CT)(t))
        _v = "a%db%d" % (_sa, _sb)
        for _form, _fn in (("dev", "zkp_add_points_dev"), ("host", "zkp_add_points")):
            for _op, _oname in ((0, "add"), (1, "sub")):
                add(_fn, _form, _n, _v + "-" + _oname, lambda f=_form, n=_n, sa=_sa, sb=_sb, op=_op: _strided_pairs("add", f, n, sa, sb, op))
        for _t in (1, 3):
            add("zkp_point_add_batch", "batch", _n, "%s-t%d" % (_v, _t),
                lambda n=_n, sa=_sa, sb=_sb, t=_t: _strided_pairs("add", "batch", n, sa, sb, 1)(t))


# ---- (6) scalars mod l ---------------------------------------------------------------------------------------------------------------------------
def _sc_invert(form, n):
    v = scalar_ints(11)[:n]
    ops = [IN("in", sc_rows(v)), OUT("out", sc_rows([pow(x % L, L - 2, L) for x in v]))]
    return (lambda t: [None, n, ops[0], t, ops[1]]) if form == "batch" else [CTX, n] + ops


@functools.lru_cache(maxsize=None)
def wide_rows(n=NMAX):
    rng = np.random.default_rng(12)
    w = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    w[0], w[1 % n] = 0, 0xff
    return w


def _sc_from_wide(form, n):
    w = wide_rows()[:n]
    ops = [IN("in", w), OUT("out", sc_rows([int.from_bytes(bytes(r), "little") % L for r in w]))]
    return (lambda t: [None, n, ops[0], t, ops[1]]) if form == "batch" else [CTX, n] + ops


def _sc_muladd(form, n, sa, sb, sc):
    """sc = None: c == NULL"""
    a, b, c = scalar_ints(13)[:n], scalar_ints(14)[::-1][:n], (scalar_ints(15)[5:] + scalar_ints(15)[:5])[:n]
    pick = lambda v, s: list(v) if s else [v[2 % n]]          # noqa: E731
    av, bv, cv = pick(a, sa), pick(b, sb), (None if sc is None else pick(c, sc))
    exp = [(av[i * sa] * bv[i * sb] + (0 if cv is None else cv[i * sc])) % L for i in range(n)]
    oa, ob, oc, out = IN("a", sc_rows(av)), IN("b", sc_rows(bv)), (None if cv is None else IN("c", sc_rows(cv))), OUT("out", sc_rows(exp))
    if form == "batch":
        return lambda t: [None, n, oa, sa, ob, sb, oc, sc or 0, t, out]
    return [CTX, n, oa, sa, ob, sb, oc, sc or 0, out]


RANDOM_KEY, RANDOM_NONCE = bytes(range(7, 39)), 0x0123456789abcdef


@functools.lru_cache(maxsize=None)
def random_scalars(n=NMAX):
    return sc_rows([int.from_bytes(chacha20_block(RANDOM_KEY, i, RANDOM_NONCE), "little") % L for i in range(n)])


def _sc_random(form, n):
    out = OUT("out", random_scalars()[:n])
    key = IN("key", np.frombuffer(RANDOM_KEY, np.uint8).reshape(1, 32), align=1)
    if form == "batch":
        return lambda t: [None, n, key, RANDOM_NONCE, t, out]
    return [CTX, n, RANDOM_KEY, RANDOM_NONCE, out] if form == "dev" else [CTX, n, key, RANDOM_NONCE, out]        # (_dev reads the key on the host)


def _hashes(kind, form, n):
    """zkp_hash_from_bytes_sha512 (kind "point") and zkp_sc_hash_from_bytes_sha512 (kind "scalar") over messages of 0, 33 and 167 bytes"""
    msgs, data, off = messages(n)
    C.build()
    if kind == "point":
        exp = PC.enc_rows([C.from_uniform_bytes(hashlib.sha512(m).digest()) for m in msgs])
    else:
        exp = sc_rows([int.from_bytes(hashlib.sha512(m).digest(), "little") % L for m in msgs])
    om, oo, out = IN("msgs", data, align=1), IN("offsets", off, align=8), OUT("out", exp)
    if form == "batch":
        return lambda t: [None, n, om, oo, t, out]
    return [CTX, n, om, len(data), oo, out] if form == "dev" else [CTX, n, om, oo, out]


@functools.lru_cache(maxsize=None)
def uniform_expected(n=NMAX):
    C.build()
    return PC.enc_rows([C.from_uniform_bytes(bytes(r)) for r in wide_rows()[:n]])


def _from_uniform(form, n):
    ops = [IN("in", wide_rows()[:n]), OUT("out", uniform_expected()[:n])]
    return (lambda t: [None, n, ops[0], t, ops[1]]) if form == "batch" else [CTX, n] + ops


for _n in ROW_SIZES:
    for _name, _b, _batch in (("sc_invert", _sc_invert, "zkp_scalar_invert_batch"), ("sc_from_wide", _sc_from_wide, "zkp_scalar_from_wide_batch"),
                              ("sc_random", _sc_random, "zkp_scalar_random_batch"), ("from_uniform_bytes", _from_uniform, "zkp_from_uniform_bytes_batch")):
        add("zkp_%s_dev" % _name, "dev", _n, "", lambda b=_b, n=_n: b("dev", n))
        add("zkp_%s" % _name, "host", _n, "", lambda b=_b, n=_n: b("host", n))
        for _t in (1, 3):
            add(_batch, "batch", _n, "t%d" % _t, lambda b=_b, n=_n, t=_t: b("batch", n)(t))
    for _kind, _name, _batch in (("point", "hash_from_bytes_sha512", "zkp_hash_from_bytes_sha512_batch"),
                                 ("scalar", "sc_hash_from_bytes_sha512", "zkp_scalar_hash_from_bytes_sha512_batch")):
        add("zkp_%s_dev" % _name, "dev", _n, "", lambda k=_kind, n=_n: _hashes(k, "dev", n))
        add("zkp_%s" % _name, "host", _n, "", lambda k=_kind, n=_n: _hashes(k, "host", n))
        for _t in (1, 3):
            add(_batch, "batch", _n, "t%d" % _t, lambda k=_kind, n=_n, t=_t: _hashes(k, "batch", n)(t))
    for _sa, _sb, _sc in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, None)):
        _v = "a%db%dc%s" % (_sa, _sb, "x" if _sc is None else _sc)
        add("zkp_sc_muladd_dev", "dev", _n, _v, lambda n=_n, s=(_sa, _sb, _sc): _sc_muladd("dev", n, *s))
        add("zkp_sc_muladd", "host", _n, _v, lambda n=_n, s=(_sa, _sb, _sc): _sc_muladd("host", n, *s))
        for _t in (1, 3):
            add("zkp_scalar_muladd_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, s=(_sa, _sb, _sc), t=_t: _sc_muladd("batch", n, *s)(t))


# ---- (3), (4) decode and encode ------------------------------------------------------------------------------------------------------------------
def _decode_check(n, with_xyzt):
    pts = PC.tiled(PC.pair_operands()[1], n)
    C.build()
    st, xyzt = C.decode_check(pts, want_coords=True)
    return [CTX, n, IN("points", pts), OUT("status", st), OUT("xyzt", xyzt) if with_xyzt else None]


def _encode_many(n):
    pts = PC.tiled(PS.pair_operands()[0][PS.pair_operands()[2]], n)
    C.build()
    st, xyzt = C.decode_check(pts, want_coords=True)
    assert not st.any()
    return [CTX, n, IN("xyzt", xyzt), OUT("out", C.encode_many(xyzt))]


for _n in ROW_SIZES:
    add("zkp_decode_check", "host", _n, "xyzt", lambda n=_n: _decode_check(n, True))
    add("zkp_decode_check", "host", _n, "", lambda n=_n: _decode_check(n, False))
    add("zkp_encode_many", "host", _n, "", lambda n=_n: _encode_many(n))


# ---- CSR calls: (1), (11), (14) multiscalar sums; (9) point sums; (12) scalar folds; (13) scans ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def msm_job(n, long_segment=0):
    """(off, scalars [T][32], pidx [T], catalogue, out [n][32], status [n]): csr_lens(n) (long_segment > 0: segment 1 has that many terms) over the
    catalogue of tests/point_sum_cases.py, whose one invalid row is referenced by one term of segment 3 (where there is one); expected from the C oracle"""
    lens = csr_lens(n)
    if long_segment:
        lens[1 if n > 1 else 0] = long_segment                # (n = 1: the long segment is the only one)
    off = SR.offsets(lens)
    t = int(off[-1])
    pts, bad = PS.catalogue()
    rng = np.random.default_rng(100 + n)
    pidx = rng.integers(0, len(pts) - 1, size=t)
    pidx[pidx >= bad] += 1
    if n > 4:
        pidx[int(off[3])] = bad
    sc = rng.integers(0, 256, size=(t, 32), dtype=np.uint8)
    C.build()
    out, st = C.msm_many(off, sc, u32(pidx), pts, 0)
    return off, sc, u32(pidx), pts, out, st


def _msm_csr(fn, form, n, with_pidx, flags, long_segment=0):
    """zkp_msm_many / zkp_msm_segments (flags) and zkp_msm_optional_many (flags = None); with_pidx False: a point per term"""
    off, sc, pidx, pts, out, st = msm_job(n, long_segment)
    t = int(off[-1])
    points = pts if with_pidx else np.ascontiguousarray(pts[pidx])
    o_off, o_sc, o_pts = IN("off", off, align=4), IN("scalars", sc), IN("points", points)
    o_pidx = IN("pidx", pidx, align=4) if with_pidx else None
    o_out, o_st = OUT("out", out), OUT("status", st, align=1)
    fl = [] if flags is None else [flags]
    if form == "batch":
        return lambda th: [None, n, o_off, o_sc, o_pidx, o_pts, len(points)] + fl + [th, o_out, o_st]
    if form == "host":
        return [CTX, n, o_off, o_sc, o_pidx, o_pts, len(points)] + fl + [o_out, o_st]
    tail = [max(csr_lens(n) + [long_segment])] if flags is None else []           # max_seg
    return [CTX, n, o_off, o_sc, o_pidx, o_pts, len(points), t] + fl + tail + [o_out, o_st]


@functools.lru_cache(maxsize=None)
def sum_job(n):
    off = SR.offsets(csr_lens(n))
    t = int(off[-1])
    pts, bad = PS.catalogue()
    rng = np.random.default_rng(200 + n)
    pidx = rng.integers(0, len(pts) - 1, size=t)
    pidx[pidx >= bad] += 1
    if n > 4:
        pidx[int(off[3]) + 1] = bad
    neg = (rng.integers(0, 3, size=t) == 0).astype(np.uint8)
    return off, u32(pidx), neg, pts


def _sum_points(form, n, with_pidx, with_neg):
    off, pidx, neg, pts = sum_job(n)
    out, st = PS.segments_expected(off, pidx, neg if with_neg else None, pts)
    points = pts if with_pidx else np.ascontiguousarray(pts[pidx])
    a = [IN("off", off, align=4), IN("pidx", pidx, align=4) if with_pidx else None, IN("neg", neg, align=1) if with_neg else None, IN("points", points)]
    o = [OUT("out", out), OUT("status", st, align=1)]
    if form == "batch":
        return lambda th: [None, n] + a + [len(points), th] + o
    return [CTX, n] + a + [len(points)] + ([int(off[-1])] if form == "dev" else []) + o


@functools.lru_cache(maxsize=None)
def scan_catalogue():
    """the rows of tests/scan_cases.py -- LOGS[i] B and one encoding that does not decode -- from the C oracle"""
    return np.ascontiguousarray(np.concatenate([DC.encode_multiples([v % L for v in SCN.LOGS]), PC.enc_rows([PC.invalid_points()[1]])]))


@functools.lru_cache(maxsize=None)
def scan_job(n):
    lens = csr_lens(n)
    bad_at = (int(SR.offsets(lens)[3]) + 7,) if n > 4 else ()
    return SCN.pt_job(lens, seed=300 + n, bad_at=bad_at)


def _scan_points(form, n, with_pidx, with_neg, exclusive):
    off, pidx, neg = scan_job(n)
    t = int(off[-1])
    logs, bad = SCN.pt_prefix_logs(off, pidx, neg if with_neg else None, exclusive)
    out = DC.encode_multiples([int(v) % L for v in logs]) if t else np.zeros((0, 32), np.uint8)
    out[bad] = 0
    cat = scan_catalogue()
    points = cat if with_pidx else np.ascontiguousarray(cat[pidx])
    a = [IN("off", off, align=4), IN("pidx", pidx, align=4) if with_pidx else None, IN("neg", neg, align=1) if with_neg else None, IN("points", points)]
    o = [OUT("out", out), OUT("status", bad.astype(np.uint8), align=1)]
    if form == "batch":
        return lambda th: [None, int(exclusive), n] + a + [len(points), th] + o
    return [CTX, int(exclusive), n] + a + [len(points)] + ([t] if form == "dev" else []) + o


@functools.lru_cache(maxsize=None)
def fold_job(n, op):
    off = SR.offsets(csr_lens(n))
    a, b = SR.operands(op, int(off[-1]), 400 + n)
    return off, a, b


def _sc_reduce(form, n, op, with_idx):
    off, a, b = fold_job(n, op)
    t = int(off[-1])
    aidx = bidx = None
    if with_idx:                                             # the operands become catalogues of 11 and 5 rows that the index lists repeat and skip
        rng = np.random.default_rng(500 + n)
        a, aidx = (a + [7] * 11)[:11], rng.integers(0, 11, size=t).astype(np.uint32)
        if b is not None:
            b, bidx = (b + [9] * 5)[:5], rng.integers(0, 5, size=t).astype(np.uint32)
    exp = SR.expected(op, off, a, aidx, b, bidx)
    args = [IN("off", off, align=4), IN("a", sc_rows(a)), len(a), None if aidx is None else IN("aidx", aidx, align=4),
            None if b is None else IN("b", sc_rows(b)), 0 if b is None else len(b), None if bidx is None else IN("bidx", bidx, align=4)]
    out = OUT("out", sc_rows(exp))
    if form == "batch":
        return lambda th: [None, op, n] + args + [th, out]
    return [CTX, op, n] + args + ([t] if form == "dev" else []) + [out]


def _sc_scan(form, n, op, with_idx, exclusive):
    off, a, _ = fold_job(n, op)
    t = int(off[-1])
    aidx = None
    if with_idx:
        a, aidx = (a + [7] * 11)[:11], np.random.default_rng(600 + n).integers(0, 11, size=t).astype(np.uint32)
    exp = SCN.sc_expected(op, off, a, aidx, exclusive)
    args = [IN("off", off, align=4), IN("a", sc_rows(a)), len(a), None if aidx is None else IN("aidx", aidx, align=4)]
    out = OUT("out", sc_rows(exp))
    if form == "batch":
        return lambda th: [None, op, int(exclusive), n] + args + [th, out]
    return [CTX, op, int(exclusive), n] + args + ([t] if form == "dev" else []) + [out]


LONG_SEGMENT = 193                     # zkp_msm_optional_many_min_segment() + 1: a bucket run, whose rows k_pip_rows writes
for _n in ROW_SIZES:
    for _wp in (True, False):
        _v = "pidx" if _wp else "nopidx"
        for _flag, _fname in ((ZKP_CT, "ct"), (ZKP_VARTIME, "vartime")):
            if _wp:                                          # zkp_msm_many has no form without pidx
                add("zkp_msm_many_dev", "dev", _n, _fname, lambda n=_n, fl=_flag: _msm_csr("many", "dev", n, True, fl))
                add("zkp_msm_many", "host", _n, _fname, lambda n=_n, fl=_flag: _msm_csr("many", "host", n, True, fl))
            add("zkp_msm_segments_dev", "dev", _n, _v + "-" + _fname, lambda n=_n, wp=_wp, fl=_flag: _msm_csr("segments", "dev", n, wp, fl))
            add("zkp_msm_segments", "host", _n, _v + "-" + _fname, lambda n=_n, wp=_wp, fl=_flag: _msm_csr("segments", "host", n, wp, fl))
        for _long in (0, LONG_SEGMENT):
            _vl = _v + ("-bucket" if _long else "")
            add("zkp_msm_optional_many_dev", "dev", _n, _vl, lambda n=_n, wp=_wp, lg=_long: _msm_csr("optional_many", "dev", n, wp, None, lg))
            add("zkp_msm_optional_many", "host", _n, _vl, lambda n=_n, wp=_wp, lg=_long: _msm_csr("optional_many", "host", n, wp, None, lg))
        for _t in (1, 3):
            if _wp:
                add("zkp_multiscalar_mul_batch", "batch", _n, "t%d" % _t, lambda n=_n, t=_t: _msm_csr("many", "batch", n, True, ZKP_VARTIME)(t))
            add("zkp_multiscalar_sum_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, wp=_wp, t=_t: _msm_csr("segments", "batch", n, wp, ZKP_CT)(t))
            add("zkp_multiscalar_optional_batch", "batch", _n, "%s-t%d" % (_v, _t),
                lambda n=_n, wp=_wp, t=_t: _msm_csr("optional_many", "batch", n, wp, None, LONG_SEGMENT)(t))
        _v = "pidx-neg" if _wp else "plain"                   # the optional arrays: both present, both NULL
        add("zkp_sum_points_dev", "dev", _n, _v, lambda n=_n, w=_wp: _sum_points("dev", n, w, w))
        add("zkp_sum_points", "host", _n, _v, lambda n=_n, w=_wp: _sum_points("host", n, w, w))
        for _ex in (False, True):
            _ve = _v + ("-exclusive" if _ex else "")
            add("zkp_scan_points_dev", "dev", _n, _ve, lambda n=_n, w=_wp, ex=_ex: _scan_points("dev", n, w, w, ex))
            add("zkp_scan_points", "host", _n, _ve, lambda n=_n, w=_wp, ex=_ex: _scan_points("host", n, w, w, ex))
        for _t in (1, 3):
            add("zkp_point_sum_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, w=_wp, t=_t: _sum_points("batch", n, w, w)(t))
            add("zkp_point_scan_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, w=_wp, t=_t: _scan_points("batch", n, w, w, t == 3)(t))
        _v = "idx" if _wp else "noidx"
        for _op, _oname in ((SR.SUM, "sum"), (SR.PRODUCT, "product"), (SR.DOT, "dot")):
            add("zkp_sc_reduce_dev", "dev", _n, "%s-%s" % (_oname, _v), lambda n=_n, op=_op, w=_wp: _sc_reduce("dev", n, op, w))
            add("zkp_sc_reduce", "host", _n, "%s-%s" % (_oname, _v), lambda n=_n, op=_op, w=_wp: _sc_reduce("host", n, op, w))
            for _t in (1, 3):
                add("zkp_scalar_reduce_batch", "batch", _n, "%s-%s-t%d" % (_oname, _v, _t), lambda n=_n, op=_op, w=_wp, t=_t: _sc_reduce("batch", n, op, w)(t))
            if _op == SR.DOT:
                continue
            for _ex in (False, True):
                _ve = "%s-%s%s" % (_oname, _v, "-exclusive" if _ex else "")
                add("zkp_sc_scan_dev", "dev", _n, _ve, lambda n=_n, op=_op, w=_wp, ex=_ex: _sc_scan("dev", n, op, w, ex))
                add("zkp_sc_scan", "host", _n, _ve, lambda n=_n, op=_op, w=_wp, ex=_ex: _sc_scan("host", n, op, w, ex))
            for _t in (1, 3):
                add("zkp_scalar_scan_batch", "batch", _n, "%s-%s-t%d" % (_oname, _v, _t),
                    lambda n=_n, op=_op, w=_wp, t=_t: _sc_scan("batch", n, op, w, t == 3)(t))


# ---- (2) one large multiscalar sum -----------------------------------------------------------------------------------------------------------------
def _msm_optional(form, n, bad):
    """n = 192: the term path, 193: the bucket path; bad: one point does not decode (*status = 1, 32 zero bytes)"""
    pts, bad_row = PS.catalogue()
    rng = np.random.default_rng(700 + n)
    pidx = rng.integers(0, len(pts) - 1, size=n)
    pidx[pidx >= bad_row] += 1
    if bad:
        pidx[n // 2] = bad_row
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    points = np.ascontiguousarray(pts[pidx])
    C.build()
    exp = C.msm_optional(sc, points)
    assert (exp is None) == bad
    word = np.array([int(bad)], np.uint32 if form == "dev" else np.int32)
    return [CTX, n, IN("scalars", sc), IN("points", points), OUT("out_point", PC.enc_rows([exp or bytes(32)])), OUT("status", word, align=4)]


for _n in (192, 193):
    for _bad in (False, True):
        add("zkp_msm_optional_dev", "dev", _n, "bad" if _bad else "", lambda n=_n, b=_bad: _msm_optional("dev", n, b))
        add("zkp_msm_optional", "host", _n, "bad" if _bad else "", lambda n=_n, b=_bad: _msm_optional("host", n, b))


# ---- (10) bounded discrete logarithms --------------------------------------------------------------------------------------------------------------
def _prepare_dlog(lib, ctx):
    assert lib.zkp_ctx_prepare_dlog(ctx, DLOG_BABY_BITS) == 0


def _prepare_dlog_point(lib, ctx):
    assert lib.zkp_ctx_prepare_dlog_point(ctx, DLOG_SLOT, DPC.base(DLOG_BASE), DLOG_BABY_BITS) == 0


def _host_baby_bits(lib, ctx):
    """the host backend's table size is a setting of the process: an 8-bit table for the call, what it was afterwards"""
    was = lib.zkp_toolbox_get_dlog_baby_bits()
    assert lib.zkp_toolbox_set_dlog_baby_bits(DLOG_BABY_BITS) == 0
    return lambda: lib.zkp_toolbox_set_dlog_baby_bits(was)


DLOG_CHUNK = 32                         # zkp_dlog_chunk(): the giant steps of one work item, which the k values of tests/dlog_cases.py sit around


def _dlog_base(form, n):
    p, k, s = DC.tiled(DLOG_BABY_BITS, DLOG_BITS, DLOG_CHUNK, n)
    ops = [IN("points", p), OUT("out", k.astype(np.uint64), align=8), OUT("status", s, align=1)]
    if form == "batch":
        return lambda t: [None, n, ops[0], DLOG_BITS, ops[1], ops[2], t]
    return [CTX, n, ops[0], DLOG_BITS, ops[1], ops[2]]


def _dlog_point(form, n, signed):
    p, k, s = DPC.tiled(DLOG_BASE, DLOG_BABY_BITS, DLOG_BITS, DLOG_CHUNK, n, signed)
    ops = [IN("points", p), OUT("out", k.astype(np.int64).view(np.uint64), align=8), OUT("status", s, align=1)]
    if form == "batch":
        return lambda t: [None, IN("base", np.frombuffer(DPC.base(DLOG_BASE), np.uint8).reshape(1, 32), align=1), n, ops[0], DLOG_BITS, int(signed), ops[1], ops[2], t]
    return [CTX, DLOG_SLOT, n, ops[0], DLOG_BITS, int(signed), ops[1], ops[2]]


for _n in ROW_SIZES:
    add("zkp_dlog_base_dev", "dev", _n, "", lambda n=_n: _dlog_base("dev", n), _prepare_dlog)
    add("zkp_dlog_base", "host", _n, "", lambda n=_n: _dlog_base("host", n), _prepare_dlog)
    for _s in (False, True):
        _v = "signed" if _s else "unsigned"
        add("zkp_dlog_point_dev", "dev", _n, _v, lambda n=_n, s=_s: _dlog_point("dev", n, s), _prepare_dlog_point)
        add("zkp_dlog_point", "host", _n, _v, lambda n=_n, s=_s: _dlog_point("host", n, s), _prepare_dlog_point)
    for _t in (1, 3):
        add("zkp_basepoint_dlog_batch", "batch", _n, "t%d" % _t, lambda n=_n, t=_t: _dlog_base("batch", n)(t), _host_baby_bits)
        add("zkp_point_dlog_batch", "batch", _n, "signed-t%d" % _t, lambda n=_n, t=_t: _dlog_point("batch", n, True)(t), _host_baby_bits)
        add("zkp_point_dlog_batch", "batch", _n, "unsigned-t%d" % _t, lambda n=_n, t=_t: _dlog_point("batch", n, False)(t), _host_baby_bits)


# ---- (7) Merlin operations on N transcripts --------------------------------------------------------------------------------------------------------
# A blob is the oracle's orc_transcript -- 200 bytes of STROBE state, pos, pos_begin, cur_flags -- and five more bytes that no operation reads.  The
# headers give those five no meaning; the catalogue expects them to come out as they went in (a blob written from a shared initial one: as that one's).
def _orc(blob):
    t = ctypes.create_string_buffer(bytes(blob[:203]), 256)
    return t


def _orc_done(t, blob):
    out = np.array(blob, np.uint8)
    out[:203] = np.frombuffer(t.raw[:203], np.uint8)
    return out


def orc_append(blob, label: bytes, msg: bytes):
    C.build()
    t = _orc(blob)
    C.lib().orc_transcript_append(t, label, msg, ctypes.c_size_t(len(msg)))
    return _orc_done(t, blob)


def orc_challenge(blob, label: bytes, n: int):
    C.build()
    t = _orc(blob)
    out = ctypes.create_string_buffer(max(n, 1))
    C.lib().orc_transcript_challenge(t, label, out, ctypes.c_size_t(n))
    return _orc_done(t, blob), out.raw[:n]


LABEL = b"footprint"


def shared_blob():
    """the one blob every transcript of a shared_initial call starts from: position 90"""
    return TO.start_states()[TR.state_at(90):][:1]


@functools.lru_cache(maxsize=None)
def _append_expected(shared, n=max(TRANSCRIPT_SIZES)):
    S = TR.tiled_states(n)
    msgs, _, _ = messages(n)
    return np.stack([orc_append(shared_blob()[0] if shared else S[j], LABEL, msgs[j]) for j in range(n)])


def _append_message(form, n, shared):
    S = TR.tiled_states(n)
    _, data, off = messages(n)
    exp = _append_expected(shared)[:n]
    om, oo = IN("msgs", data, align=1), IN("offsets", off, align=8)
    if form == "dev":
        if shared:
            return [CTX, n, 1, IN("ts_in", shared_blob()), OUT("ts_out", exp), LABEL, om, len(data), oo]
        ts = INOUT("ts", S, exp)
        return [CTX, n, 0, ts, ts, LABEL, om, len(data), oo]
    start = S.copy()
    if shared:
        start[0] = shared_blob()[0]                                      # ts[0] is the blob every transcript starts from; the other rows are overwritten
        start[1:] = prefill(208 * (n - 1)).reshape(n - 1, 208)
    ts = INOUT("ts", start, exp)
    if form == "batch":
        return lambda t, with_ctx: ([None] if with_ctx else []) + [ts, n, int(shared), LABEL, om, oo, t]
    return [CTX, n, int(shared), ts, LABEL, om, oo]


@functools.lru_cache(maxsize=None)
def _challenge_expected(length, n=max(TRANSCRIPT_SIZES)):
    S = TR.tiled_states(n)
    pairs = [orc_challenge(S[j], LABEL, length) for j in range(n)]
    return np.stack([p[0] for p in pairs]), np.frombuffer(b"".join(p[1] for p in pairs), np.uint8).reshape(n, length)


def _challenge_bytes(form, n, length):
    adv, out = _challenge_expected(length)
    ts, o = INOUT("ts", TR.tiled_states(n), adv[:n]), OUT("out", out[:n], align=1)
    if form == "batch":
        return lambda t: [None, ts, n, LABEL, length, t, o]
    return [CTX, n, ts, LABEL, length, o]


@functools.lru_cache(maxsize=None)
def _challenge_scalars_expected(n=max(TRANSCRIPT_SIZES)):
    adv, out = _challenge_expected(64)
    return adv, sc_rows([int.from_bytes(bytes(r), "little") % L for r in out])


def _challenge_scalars(form, n):
    adv, out = _challenge_scalars_expected()
    ts, o = INOUT("ts", TR.tiled_states(n), adv[:n]), OUT("out", out[:n], align=1)
    if form == "batch":
        return lambda t: [None, ts, n, LABEL, t, o]
    return [CTX, n, ts, LABEL, o]


KIND, VAR = b"ptvar", b"Q"


@functools.lru_cache(maxsize=None)
def _append_points_expected(validate, n=max(TRANSCRIPT_SIZES)):
    S = TR.tiled_states(n)
    pts = TR.points(n, zero_rows=(0, 5, 32, 64, 256))
    out, st = [], []
    for j in range(n):
        rejected = bool(validate) and not pts[j].any()
        out.append(S[j] if rejected else orc_append(orc_append(S[j], KIND, VAR), b"val", bytes(pts[j])))
        st.append(rejected)
    return pts, np.stack(out), np.array(st, np.uint8)


def _append_points(form, n, validate, with_status):
    pts, adv, st = _append_points_expected(validate)
    ts, p, s = INOUT("ts", TR.tiled_states(n), adv[:n]), IN("points", pts[:n], align=1), (OUT("status", st[:n], align=1) if with_status else None)
    if form == "batch":
        return lambda t: [None, ts, n, KIND, VAR, p, validate, t, s]
    return [CTX, n, ts, KIND, VAR, p, validate, s]


RNG_M, RNG_WLEN, RNG_COUNT = 1, 32, {0: 2, 1: 33}            # one 32-byte witness; two scalars, or 33 bytes


def _model_strobe(blob):
    s = object.__new__(M.Strobe128)
    s.state = bytearray(bytes(blob[:200]))
    s.pos, s.pos_begin, s.cur_flags = int(blob[200]), int(blob[201]), int(blob[202])
    return s


@functools.lru_cache(maxsize=None)
def _witness_rng_expected(mode, n=max(TRANSCRIPT_SIZES)):
    """oracle.model's TranscriptRng: build_rng, rekey_with_witness_bytes per witness, finalize, then Scalar::random x count or one fill_bytes"""
    S, W, E = TR.tiled_states(n), TR.witnesses(n, RNG_M, RNG_WLEN), TR.entropy(n)
    rows = []
    for j in range(n):
        b = M.TranscriptRngBuilder(_model_strobe(S[j]))
        for k in range(RNG_M):
            b.rekey_with_witness_bytes(LABEL, bytes(W[j, k]))
        rng = b.finalize(bytes(E[j]))
        rows.append(b"".join(M.sc_to_bytes(rng.random_scalar()) for _ in range(RNG_COUNT[0])) if mode == 0 else rng.fill_bytes(RNG_COUNT[1]))
    return np.frombuffer(b"".join(rows), np.uint8).reshape(n, -1).copy()


def _witness_rng(form, n, mode):
    ts, w, e = IN("ts", TR.tiled_states(n)), IN("witnesses", TR.witnesses(n, RNG_M, RNG_WLEN).reshape(n, -1), align=1), IN("entropy", TR.entropy(n), align=1)
    out = OUT("out", _witness_rng_expected(mode)[:n], align=1)
    if form == "batch":
        return lambda t: [None, ts, n, LABEL, RNG_M, RNG_WLEN, w, e, mode, RNG_COUNT[mode], t, out]
    return [CTX, n, ts, LABEL, RNG_M, RNG_WLEN, w, e, mode, RNG_COUNT[mode], out]


for _n in TRANSCRIPT_SIZES:
    for _sh in (0, 1):
        _v = "shared" if _sh else "inplace"
        add("zkp_transcripts_append_message_dev", "dev", _n, _v, lambda n=_n, sh=_sh: _append_message("dev", n, sh))
        add("zkp_transcripts_append_message", "host", _n, _v, lambda n=_n, sh=_sh: _append_message("host", n, sh))
        for _t in (1, 3):
            add("zkp_transcripts_append_message_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, sh=_sh, t=_t: _append_message("batch", n, sh)(t, False))
            add("zkp_transcripts_append_message_batch_ctx", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, sh=_sh, t=_t: _append_message("batch", n, sh)(t, True))
    for _len in (0, 1, 167):
        add("zkp_transcripts_challenge_bytes_dev", "dev", _n, "len%d" % _len, lambda n=_n, ln=_len: _challenge_bytes("dev", n, ln))
        add("zkp_transcripts_challenge_bytes", "host", _n, "len%d" % _len, lambda n=_n, ln=_len: _challenge_bytes("host", n, ln))
        for _t in (1, 3):
            add("zkp_transcripts_challenge_bytes_batch", "batch", _n, "len%d-t%d" % (_len, _t), lambda n=_n, ln=_len, t=_t: _challenge_bytes("batch", n, ln)(t))
    add("zkp_transcripts_challenge_scalars_dev", "dev", _n, "", lambda n=_n: _challenge_scalars("dev", n))
    add("zkp_transcripts_challenge_scalars", "host", _n, "", lambda n=_n: _challenge_scalars("host", n))
    for _val, _ws, _v in ((0, False, "nostatus"), (0, True, "status"), (1, True, "validate")):
        add("zkp_transcripts_append_points_dev", "dev", _n, _v, lambda n=_n, va=_val, ws=_ws: _append_points("dev", n, va, ws))
        add("zkp_transcripts_append_points", "host", _n, _v, lambda n=_n, va=_val, ws=_ws: _append_points("host", n, va, ws))
        for _t in (1, 3):
            add("zkp_transcripts_append_points_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, va=_val, ws=_ws, t=_t: _append_points("batch", n, va, ws)(t))
    for _mode, _v in ((0, "scalars"), (1, "bytes")):
        add("zkp_transcripts_witness_rng_dev", "dev", _n, _v, lambda n=_n, m=_mode: _witness_rng("dev", n, m))
        add("zkp_transcripts_witness_rng", "host", _n, _v, lambda n=_n, m=_mode: _witness_rng("host", n, m))
        for _t in (1, 3):
            add("zkp_transcripts_witness_rng_batch", "batch", _n, "%s-t%d" % (_v, _t), lambda n=_n, m=_mode, t=_t: _witness_rng("batch", n, m)(t))
    for _t in (1, 3):
        add("zkp_transcripts_challenge_scalars_batch", "batch", _n, "t%d" % _t, lambda n=_n, t=_t: _challenge_scalars("batch", n)(t))


# ---- (5) hash to the group from a transcript; the ChaCha20 stream ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hash_to_group_expected(aligned, n=max(TRANSCRIPT_SIZES)):
    """N x { challenge_bytes(label, 64) ; from_uniform_bytes }; aligned: every transcript is the blob at position 90"""
    C.build()
    if aligned:
        adv, out = orc_challenge(shared_blob()[0], LABEL, 64)
        return np.repeat(shared_blob(), n, axis=0), np.stack([adv] * n), PC.enc_rows([C.from_uniform_bytes(out)] * n)
    adv, out = _challenge_expected(64)
    return TR.tiled_states(n), adv, PC.enc_rows([C.from_uniform_bytes(bytes(r)) for r in out])


def _hash_to_group(form, n, aligned):
    start, adv, out = _hash_to_group_expected(aligned)
    ts, o = INOUT("transcripts", start[:n], adv[:n]), OUT("out", out[:n])
    if form == "batch":
        return lambda t: [None, n, ts, LABEL, t, o]
    return [CTX, n, ts, LABEL, o]


FILL_FIRST_BLOCK = 5


@functools.lru_cache(maxsize=None)
def _fill_expected(n=NMAX):
    return np.frombuffer(b"".join(chacha20_block(RANDOM_KEY, FILL_FIRST_BLOCK + b, RANDOM_NONCE) for b in range(n)), np.uint8).reshape(n, 64).copy()


for _n in TRANSCRIPT_SIZES:
    add("zkp_fused_hash_to_group", "host", _n, "", lambda n=_n: _hash_to_group("host", n, True))
    add("zkp_fused_hash_to_group_ragged", "host", _n, "", lambda n=_n: _hash_to_group("host", n, False))
    for _t in (1, 3):
        add("zkp_hash_to_group_batch", "batch", _n, "t%d" % _t, lambda n=_n, t=_t: _hash_to_group("batch", n, False)(t))
for _n in ROW_SIZES:                     # n blocks of 64 bytes (the key is read on the host)
    add("zkp_chacha20_fill_dev", "dev", _n, "", lambda n=_n: [CTX, RANDOM_KEY, RANDOM_NONCE, FILL_FIRST_BLOCK, OUT("out", _fill_expected()[:n]), 64 * n])


# ---- the statement flows of the toolbox on the host backend: DLEQ proofs -----------------------------------------------------------------------------
PROOF_LABEL = b"footprint proofs"


SEED = bytes(range(101, 141))              # key [32] || nonce [8] of the seeded flows


def seed_stream(n_bytes):
    """the first n_bytes of the ChaCha20 stream the seeded flows draw from"""
    nonce = int.from_bytes(SEED[32:], "little")
    return np.frombuffer(b"".join(chacha20_block(SEED[:32], b, nonce) for b in range((n_bytes + 63) // 64)), np.uint8)[:n_bytes].copy()


@functools.lru_cache(maxsize=None)
def dleq_batch(kind="aligned", n=max(TRANSCRIPT_SIZES)):
    """n DLEQ proofs (A = x G, B = x H) from the C oracle's prover, and the transcripts as the reference leaves them: the appends of
    Prover::new, allocate_scalar, allocate_point, the blinding commitments and the challenge draw (src/toolbox/prover.rs, mod.rs:165-228)
    restated over the oracle's Merlin -- the restatement is checked against the challenge the oracle's own prover returns.  kind "seeded": the
    prover's entropy is the stream of SEED; "ragged": the transcript labels have three lengths, so the blobs stand at three STROBE positions"""
    C.build()
    rng = np.random.default_rng(900)
    x = rng.integers(0, 256, size=(n, 1, 32), dtype=np.uint8)
    x[:, :, 31] &= 0x0f
    G = PC.BASEPOINT_ROW
    H = PC.tiled(PC.enc_rows(PC.hashed_points()), n)
    A, _ = oracle_products(x[:, 0], np.repeat(G, n, axis=0))
    B, _ = oracle_products(x[:, 0], H)
    inst = np.ascontiguousarray(np.stack([A, B, H]))
    entropy = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if kind == "seeded":
        entropy = seed_stream(32 * n).reshape(n, 32)
    cst = C.Statement.from_model(M.dleq_statement())
    chal, resp, coms, adv, start = [], [], [], [], []
    for j in range(n):
        label = PROOF_LABEL + b"+" * (j % 3 if kind == "ragged" else 0)
        t0 = ctypes.create_string_buffer(256)
        C.lib().orc_transcript_init(t0, label, ctypes.c_size_t(len(label)))
        blob0 = np.zeros(208, np.uint8)
        blob0[:203] = np.frombuffer(t0.raw[:203], np.uint8)
        start.append(blob0)
        c, r, k, _ = C.prove(cst, label, x[j], np.concatenate([inst[:, j], G]), entropy[j].tobytes())
        b = orc_append(orc_append(blob0, b"dom-sep", b"schnorrzkp/1.0/ristretto255"), b"dom-sep", b"DLEQ proof")
        b = orc_append(b, b"scvar", b"x")
        for name, enc in ((b"A", A[j]), (b"B", B[j]), (b"H", H[j]), (b"G", G[0])):
            b = orc_append(orc_append(b, b"ptvar", name), b"val", bytes(enc))
        for name, enc in ((b"A", k[0]), (b"B", k[1])):
            b = orc_append(orc_append(b, b"blindcom", name), b"val", bytes(enc))
        b, wide = orc_challenge(b, b"chal", 64)
        assert int.from_bytes(wide, "little") % L == int.from_bytes(bytes(c), "little"), "the transcript restatement disagrees with the oracle's prover"
        chal.append(c); resp.append(r); coms.append(k); adv.append(b)
    return dict(x=x, inst=inst, common=G.copy(), entropy=entropy, ts0=np.stack(start), ts1=np.stack(adv),
                chal=np.stack(chal), resp=np.stack(resp), coms=np.stack(coms))


@functools.lru_cache(maxsize=None)
def _dleq_handle():
    from zkp_amd import toolbox as T
    return T.dleq_module()                # (kept alive: its statement handle goes into the calls)


def _prove_batch(n, t):
    d = dleq_batch()
    inst = np.ascontiguousarray(d["inst"][:, :n])
    return [None, _dleq_handle().statement._h, n, INOUT("transcripts", d["ts0"][:n], d["ts1"][:n]), IN("secrets", d["x"][:n].reshape(n, -1)),
            IN("inst_points", inst.reshape(3, -1)), IN("common_points", d["common"]), IN("entropy", d["entropy"][:n]), t,
            OUT("challenges", d["chal"][:n]), OUT("responses", d["resp"][:n].reshape(n, -1)), OUT("commitments", d["coms"][:n].reshape(n, -1))]


def _verify_compact_batch(n, t):
    d = dleq_batch()
    inst = np.ascontiguousarray(d["inst"][:, :n])
    return [None, _dleq_handle().statement._h, n, INOUT("transcripts", d["ts0"][:n], d["ts1"][:n]), IN("inst_points", inst.reshape(3, -1)),
            IN("common_points", d["common"]), IN("challenges", d["chal"][:n]), IN("responses", d["resp"][:n].reshape(n, -1)), t,
            OUT("results", np.zeros(n, np.uint8))]


for _n in TRANSCRIPT_SIZES:
    for _t in (1, 3):
        add("zkp_prove_batch", "batch", _n, "dleq-t%d" % _t, lambda n=_n, t=_t: _prove_batch(n, t))
        add("zkp_verify_compact_batch", "batch", _n, "dleq-t%d" % _t, lambda n=_n, t=_t: _verify_compact_batch(n, t))


# ---- (2b), (2c), (2d) the fused statement flows, and the toolbox's batchable verifiers on the host backend: DLEQ proofs ------------------------------
# Every flow gets the proofs of dleq_batch(): valid proofs, so every verdict row is 0 and every transcript ends where the prover's ended (the
# verifiers append the same points, recompute or read the same commitments and draw the same challenge).  Coefficient vectors and the operand
# list of the batch MSM come from the C oracle's batch verifier (batch_verifier.rs:173-228), which stops in front of the MSM when asked for them.
# N x K: the proofs of a many-batch call are the first N of the batch, cut into K batches.
MANY = {1: (1, 1), 33: (3, 11), 65: (5, 13), 257: (1, 257)}         # N -> (n_batches, N_each)
NS, NI, NC, NSEC = 1, 3, 2, 1                                        # DLEQ: static and instance points, constraints, secrets


@functools.lru_cache(maxsize=None)
def _fused_statement():
    from zkp_amd.engine import FusedStatement
    return FusedStatement(b"DLEQ proof", [b"x"], [(b"A", False), (b"B", False), (b"H", False), (b"G", True)], [(0, [(0, 3)]), (1, [(0, 2)])])


def FST():
    return ctypes.byref(_fused_statement().c)


@functools.lru_cache(maxsize=None)
def weights(n=max(TRANSCRIPT_SIZES)):
    """[N][nc][16]: proof j's factors; a batch call over the first n proofs takes them as [nc][n][16]"""
    return np.random.default_rng(901).integers(0, 256, size=(n, NC, 16), dtype=np.uint8)


def batch_weights(n, w=None):
    return np.ascontiguousarray((weights() if w is None else w)[:n].transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def batch_operands(lo, hi, seeded=False):
    """(coefficients, points), each [ns + (ni + nc) n][32], of one batch verification of the proofs [lo, hi) from the C oracle"""
    d = dleq_batch()
    n = hi - lo
    w = seed_stream(16 * NC * max(TRANSCRIPT_SIZES)) if seeded else None
    cst = C.Statement.from_model(M.dleq_statement())
    wb = np.ascontiguousarray(weights()[lo:hi].transpose(1, 0, 2)) if w is None else w
    rc, ms, mp = C.batch_verify(cst, PROOF_LABEL, n, np.ascontiguousarray(d["inst"][:, lo:hi]), d["common"], d["coms"][lo:hi], d["resp"][lo:hi], wb,
                                want_msm_inputs=True)
    assert rc == 0
    return ms, mp


def many_coefficients(k, n_each):
    """debug_scalars of a many-batch call: the static coefficients batch by batch, then the matrix row-major over all N proofs"""
    parts = [batch_operands(b * n_each, (b + 1) * n_each)[0] for b in range(k)]
    static = [p[:NS] for p in parts]
    rows = [np.concatenate([p[NS + r * n_each:NS + (r + 1) * n_each] for p in parts]) for r in range(NI + NC)]
    return np.ascontiguousarray(np.concatenate(static + rows))


@functools.lru_cache(maxsize=None)
def each_coefficients(n=max(TRANSCRIPT_SIZES)):
    """[N][ns + ni + nc][32]: what verifier.rs:144-160 folds per proof -- a batch verification of that one proof with its own factors"""
    d = dleq_batch()
    cst = C.Statement.from_model(M.dleq_statement())
    out = []
    for j in range(n):
        rc, ms, _ = C.batch_verify(cst, PROOF_LABEL, 1, np.ascontiguousarray(d["inst"][:, j:j + 1]), d["common"], d["coms"][j:j + 1], d["resp"][j:j + 1],
                                   np.ascontiguousarray(weights()[j:j + 1].transpose(1, 0, 2)), want_msm_inputs=True)
        assert rc == 0
        out.append(ms)
    return np.stack(out)


def flat(a, n):
    return np.ascontiguousarray(a).reshape(n, -1)


def _proof_ops(n, kind="aligned"):
    """the operands every flow draws from, over the first n proofs"""
    d = dleq_batch(kind)
    o = dict(d=d, n=n)
    o["ts"] = lambda: INOUT("transcripts", d["ts0"][:n], d["ts1"][:n])
    o["ts_in"] = lambda: IN("transcripts", d["ts0"][:n])
    o["ts_out"] = lambda: OUT("transcripts_out", d["ts1"][:n])
    o["secrets"] = IN("secrets", flat(d["x"][:n], n))
    o["inst"] = IN("inst", flat(d["inst"][:, :n], NI))
    o["common"] = IN("common", d["common"])
    o["entropy"] = IN("entropy", d["entropy"][:n])
    o["chal_in"], o["resp_in"], o["coms_in"] = IN("challenges", d["chal"][:n]), IN("responses", flat(d["resp"][:n], n)), IN("commitments", flat(d["coms"][:n], n))
    o["chal"], o["resp"], o["coms"] = OUT("challenges", d["chal"][:n]), OUT("responses", flat(d["resp"][:n], n)), OUT("commitments", flat(d["coms"][:n], n))
    o["w_each"] = IN("weights16", flat(weights()[:n], n), align=16)
    o["w_batch"] = IN("weights16", flat(batch_weights(n), NC), align=16)
    o["results"] = lambda: OUT("results", np.zeros(n, np.uint8))
    o["word"] = lambda name, k=1: OUT(name, np.zeros(k, np.int32), align=4)
    o["table"] = np.concatenate([d["common"], d["inst"][:, :n].reshape(-1, 32)])
    o["pos"] = TO.pos_word(d["ts0"][0])
    return o


def _fused_prove(fn, n):
    kind = {"zkp_fused_prove_seeded": "seeded", "zkp_fused_prove_ragged": "ragged"}.get(fn, "aligned")
    o = _proof_ops(n, kind)
    rng = {"zkp_fused_prove": [o["entropy"]], "zkp_fused_prove_seeded": [SEED], "zkp_fused_prove_ragged": [o["entropy"], None]}[fn]
    return [CTX, FST(), n, o["ts"](), o["secrets"], o["inst"], o["common"]] + rng + [o["chal"], o["resp"], o["coms"], o["word"]("invalid_point")]


def _fused_verify_compact(fn, n):
    o = _proof_ops(n, "ragged" if fn.endswith("ragged") else "aligned")
    return [CTX, FST(), n, o["ts"](), o["inst"], o["common"], o["chal_in"], o["resp_in"], o["results"]()]


def _fused_verify_batchable(fn, n, with_debug=False):
    o = _proof_ops(n, "ragged" if fn.endswith("ragged") else "aligned")
    tail = [OUT("debug_scalars", flat(each_coefficients()[:n], n)) if with_debug else None] if fn.endswith("coeffs") else []
    return [CTX, FST(), n, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"], o["w_each"], o["results"]()] + tail


def _fused_batch_verify(n, with_debug):
    o = _proof_ops(n)
    return [CTX, FST(), n, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"], o["w_batch"], o["word"]("verdict"),
            OUT("debug_scalars", batch_operands(0, n)[0]) if with_debug else None]


def many_weights(k, n_each):
    """[nc][N][16] of a many-batch call: proof j keeps its own factors, as in the single batches the oracle verifies"""
    return IN("weights16", flat(batch_weights(k * n_each), NC), align=16)


def _fused_batch_verify_many(fn, n, with_debug=False):
    k, n_each = MANY[n]
    o = _proof_ops(n, "ragged" if fn.endswith("ragged") else "aligned")
    head = [CTX, FST(), k, n_each, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"]]
    verdicts = o["word"]("verdicts", k)
    if fn.endswith("seeded"):
        return head + [SEED, verdicts]
    if fn.endswith("ragged"):
        return head + [many_weights(k, n_each), None, verdicts]
    return head + [many_weights(k, n_each), verdicts, OUT("debug_scalars", many_coefficients(k, n_each)) if with_debug else None]


def _batch_check(n, with_debug):
    o = _proof_ops(n)
    d = o["d"]
    minus_c = sc_rows([(L - int.from_bytes(bytes(c), "little")) % L for c in d["chal"][:n]])
    return [CTX, ctypes.byref(_fused_statement().c.shape), n, IN("minus_c", minus_c), o["resp_in"], o["w_batch"], IN("static_points", d["common"]), o["inst"],
            o["coms_in"], OUT("out_point", np.zeros((1, 32), np.uint8)), o["word"]("status"), OUT("debug_scalars", batch_operands(0, n)[0]) if with_debug else None]


def _fused_submit(fn, n, with_ts_out):
    """the flows as asynchronous jobs on host buffers: submit, then zkp_ctx_job_wait; the incoming transcripts are read only"""
    o = _proof_ops(n)
    ts_out = o["ts_out"]() if with_ts_out else None
    if fn == "zkp_fused_prove_submit":
        return [CTX, FST(), n, 0, o["ts_in"](), o["secrets"], o["inst"], n, o["common"], o["entropy"], None, ts_out, o["chal"], o["resp"], o["coms"],
                o["word"]("invalid_point")]
    if fn == "zkp_fused_verify_compact_submit":
        return [CTX, FST(), n, 0, o["ts_in"](), o["inst"], n, o["common"], o["chal_in"], o["resp_in"], ts_out, o["results"]()]
    if fn == "zkp_fused_verify_batchable_submit":
        return [CTX, FST(), n, 0, o["ts_in"](), o["inst"], n, o["common"], o["coms_in"], o["resp_in"], o["w_each"], None, ts_out, o["results"]()]
    k, n_each = MANY[n]
    return [CTX, FST(), k, n_each, 0, o["ts_in"](), o["inst"], n, o["common"], o["coms_in"], o["resp_in"], many_weights(k, n_each), n, None, ts_out,
            o["word"]("verdicts", k)]


def _fused_dev(fn, n):
    """the device-resident flows: every buffer 16-byte aligned; d_table = common points, then the instance rows"""
    o = _proof_ops(n)
    d = o["d"]
    a16 = lambda name, arr: IN(name, arr, align=16)                   # noqa: E731
    ts, table = INOUT("d_transcripts", d["ts0"][:n], d["ts1"][:n]), a16("d_table", o["table"])
    if fn == "zkp_fused_prove_dev":
        return [CTX, FST(), n, o["pos"], ts, o["secrets"], table, o["entropy"], o["chal"], o["resp"], o["coms"],
                OUT("d_status", np.zeros(n * NC, np.uint8), align=16)]
    if fn == "zkp_fused_verify_compact_dev":
        return [CTX, FST(), n, o["pos"], ts, table, o["chal_in"], o["resp_in"], OUT("d_results", np.zeros(n, np.uint8), align=16)]
    if fn == "zkp_fused_verify_batchable_dev":
        full = a16("d_table", np.concatenate([o["table"], d["coms"][:n].reshape(-1, 32)]))
        return [CTX, FST(), n, o["pos"], ts, full, o["resp_in"], o["w_each"], OUT("d_results", np.zeros(n, np.uint8), align=16)]
    # batch verification: d_points comes with the static points and the instance rows, the call writes the commitment rows behind them
    k, n_each = MANY[n] if fn.endswith("many_dev") else (1, n)
    points = np.concatenate([o["table"], np.stack([d["coms"][:n, c] for c in range(NC)]).reshape(-1, 32)])
    assert k > 1 or (points == batch_operands(0, n)[1]).all(), "the operand list disagrees with the oracle's"
    given = points.copy()
    given[len(o["table"]):] = 0xEE
    pts = INOUT("d_points", given, points)
    tail = [pts, o["coms_in"], o["resp_in"], many_weights(k, n_each), OUT("d_out_points", np.zeros((k, 32), np.uint8)),
            OUT("d_status", np.zeros((k, 2), np.uint32), align=16)]
    return [CTX, FST()] + ([k, n_each] if fn.endswith("many_dev") else [n]) + [o["pos"], ts] + tail


for _n in TRANSCRIPT_SIZES:
    for _fn in ("zkp_fused_prove", "zkp_fused_prove_seeded", "zkp_fused_prove_ragged"):
        add(_fn, "host", _n, "", lambda fn=_fn, n=_n: _fused_prove(fn, n))
    for _fn in ("zkp_fused_verify_compact", "zkp_fused_verify_compact_ragged"):
        add(_fn, "host", _n, "", lambda fn=_fn, n=_n: _fused_verify_compact(fn, n))
    for _fn in ("zkp_fused_verify_batchable", "zkp_fused_verify_batchable_ragged"):
        add(_fn, "host", _n, "", lambda fn=_fn, n=_n: _fused_verify_batchable(fn, n))
    for _dbg in (False, True):
        _v = "debug" if _dbg else ""
        add("zkp_fused_verify_batchable_coeffs", "host", _n, _v, lambda n=_n, g=_dbg: _fused_verify_batchable("zkp_fused_verify_batchable_coeffs", n, g))
        add("zkp_fused_batch_verify", "host", _n, _v, lambda n=_n, g=_dbg: _fused_batch_verify(n, g))
        add("zkp_fused_batch_verify_many", "host", _n, _v, lambda n=_n, g=_dbg: _fused_batch_verify_many("zkp_fused_batch_verify_many", n, g))
        add("zkp_batch_check", "host", _n, _v, lambda n=_n, g=_dbg: _batch_check(n, g))
    for _fn in ("zkp_fused_batch_verify_many_seeded", "zkp_fused_batch_verify_many_ragged"):
        add(_fn, "host", _n, "", lambda fn=_fn, n=_n: _fused_batch_verify_many(fn, n))
    for _fn in ("zkp_fused_prove_submit", "zkp_fused_verify_compact_submit", "zkp_fused_verify_batchable_submit", "zkp_fused_batch_verify_many_submit"):
        for _tso in (False, True):
            add(_fn, "host", _n, "tsout" if _tso else "", lambda fn=_fn, n=_n, t=_tso: _fused_submit(fn, n, t), finish="zkp_ctx_job_wait")
    for _fn in ("zkp_fused_prove_dev", "zkp_fused_verify_compact_dev", "zkp_fused_verify_batchable_dev", "zkp_fused_batch_verify_dev",
                "zkp_fused_batch_verify_many_dev"):
        add(_fn, "dev", _n, "", lambda fn=_fn, n=_n: _fused_dev(fn, n))


# the toolbox's batchable verifiers on the host backend (ctx == NULL)
def _toolbox_verify(fn, n, t):
    o = _proof_ops(n)
    st = _dleq_handle().statement._h
    if fn == "zkp_verify_batchable_each":
        return [None, st, n, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"], o["w_each"], t, o["results"]()]
    if fn == "zkp_batch_verify_many":
        k, n_each = MANY[n]
        return [None, st, k, n_each, n, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"], many_weights(k, n_each), t, o["word"]("verdicts", k)]
    tail = {"zkp_batch_verify": [], "zkp_batch_verify_locate": [o["results"]()],
            "zkp_batch_verify_coeffs": [OUT("coeffs", batch_operands(0, n)[0])]}[fn]
    return [None, st, n, n, o["ts"](), o["inst"], o["common"], o["coms_in"], o["resp_in"], o["w_batch"], t] + tail


for _n in TRANSCRIPT_SIZES:
    for _t in (1, 3):
        for _fn in ("zkp_verify_batchable_each", "zkp_batch_verify", "zkp_batch_verify_many", "zkp_batch_verify_locate", "zkp_batch_verify_coeffs"):
            add(_fn, "batch", _n, "dleq-t%d" % _t, lambda fn=_fn, n=_n, t=_t: _toolbox_verify(fn, n, t))

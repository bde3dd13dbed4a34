"""One small call per host-pointer entry point that stages its arguments through the device workspace, for tests/test_gpu_staged_ws_bytes.py (which
pins the workspace each call asks for) and tools/record_staged_ws_bytes.py (which records it).  CASES: name -> call(engine); the engine is a fresh
test-hook context, the call is the only one that touches its workspace.

Sizes: n = 257 for the per-item calls (odd, more than one block); both strides of every strided operand; three segments of 0, 1 and 300 terms for
the CSR calls, with and without their optional index / sign arrays; zkp_msm_optional on both sides of kSmallOptional and at the smallest n of every
window size pick_c knows; zkp_msm_many on both sides of the 1,024 terms at which it classifies its points; two messages, one empty, that start at
offsets[0] = 5 for the hash and append calls.  The workspace size depends on the shapes alone, so the operands are as plain as they can be: the
identity's encoding (32 zero bytes, a valid point), zero scalars, zeroed transcripts (position 0)."""
import numpy as np

from zkp_amd.engine import ZKP_CT, ZKP_RNG_SCALARS, ZKP_SC_DOT, ZKP_SC_PRODUCT, ZKP_SC_SUM, ZKP_VARTIME

N = 257
SMALL_OPTIONAL = 192                                    # kSmallOptional (csrc/zkp_kernels.hip)
PICK_C_FIRST = {7: SMALL_OPTIONAL + 1, 10: 1 << 12, 11: 1 << 13, 16: 1 << 21}        # pick_c: the smallest n of each window size
OFF = np.array([0, 0, 1, 301], np.uint32)               # segments of 0, 1 and 300 terms
T = int(OFF[-1])
N_PTS = 7                                               # the points the indexed forms draw from
BASE = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")      # the ristretto255 basepoint


def rows(n, width=32):
    return np.zeros((n, width), np.uint8)


def idx(n_terms, bound):
    return (np.arange(n_terms, dtype=np.uint32) % bound).astype(np.uint32)


def shared(stride, n):
    """an operand of n rows (stride 1) or one row for all (stride 0)"""
    return rows(n) if stride else rows(1)


MSGS = (np.zeros(5 + 70, np.uint8), np.array([5, 5, 75], np.uint64))         # messages of 0 and 70 bytes, the first 5 bytes of data unused


def _msm_many(n_terms):
    off = np.array([0, 0, 1, n_terms], np.uint32)
    return lambda e: e.msm_many(off, rows(n_terms), idx(n_terms, N_PTS), rows(N_PTS), ZKP_CT)


def _dlog_point(signed):
    def call(e):
        e.prepare_dlog_point(0, BASE, 4)
        e.dlog_point(0, rows(N), 8, signed=signed)
    return call


def _dlog_base(e):
    e.prepare_dlog(4)
    e.dlog_base(rows(N), 8)


CASES = {}
for n_terms in (1023, 1024):
    CASES["msm_many[%d]" % n_terms] = _msm_many(n_terms)
for flags, fname in ((ZKP_CT, "ct"), (ZKP_VARTIME, "vartime")):
    CASES["msm_segments[pidx,%s]" % fname] = lambda e, flags=flags: e.msm_segments(OFF, rows(T), rows(N_PTS), idx(T, N_PTS), flags)
    CASES["msm_segments[%s]" % fname] = lambda e, flags=flags: e.msm_segments(OFF, rows(T), rows(T), None, flags)
for n in (0, SMALL_OPTIONAL, SMALL_OPTIONAL + 1) + tuple(PICK_C_FIRST[c] for c in (10, 11, 16)):
    CASES["msm_optional[%d]" % n] = lambda e, n=n: e.msm_optional(rows(n), rows(n))
CASES["decode_check"] = lambda e: e.decode_check(rows(N))
CASES["decode_check[coords]"] = lambda e: e.decode_check(rows(N), want_coords=True)
CASES["encode_many"] = lambda e: e.encode_many(rows(N, 128))
CASES["from_uniform_bytes"] = lambda e: e.from_uniform_bytes(rows(N, 64))
CASES["hash_from_bytes_sha512"] = lambda e: e.hash_from_bytes_sha512_csr(*MSGS)
CASES["sc_hash_from_bytes_sha512"] = lambda e: e.scalar_hash_from_bytes_sha512_csr(*MSGS)
CASES["debug_sha512"] = lambda e: e.debug_sha512(*MSGS)
CASES["sc_invert"] = lambda e: e.scalar_invert(rows(N))
CASES["sc_from_wide"] = lambda e: e.scalar_from_wide(rows(N, 64))
for sa in (0, 1):
    for sb in (0, 1):
        for sc in (None, 0, 1):
            if (sa, sb, sc) in ((0, 0, 0), (0, 0, None)):
                continue                                # every operand shared: n = 1, not a call of 257 rows
            CASES["sc_muladd[%d,%d,%s]" % (sa, sb, sc)] = lambda e, sa=sa, sb=sb, sc=sc: e.scalar_muladd(
                shared(sa, N), shared(sb, N), None if sc is None else shared(sc, N))
        if sa or sb:
            CASES["mul_points[%d,%d]" % (sa, sb)] = lambda e, sa=sa, sb=sb: e.mul_points(shared(sa, N), shared(sb, N))
            CASES["add_points[%d,%d]" % (sa, sb)] = lambda e, sa=sa, sb=sb: e.add_points(shared(sa, N), shared(sb, N))
for op, oname in ((ZKP_SC_SUM, "sum"), (ZKP_SC_PRODUCT, "product")):
    CASES["sc_reduce[%s]" % oname] = lambda e, op=op: e.scalar_reduce(op, OFF, rows(T))
    CASES["sc_reduce[%s,aidx]" % oname] = lambda e, op=op: e.scalar_reduce(op, OFF, rows(N_PTS), idx(T, N_PTS))
    CASES["sc_scan[%s]" % oname] = lambda e, op=op: e.scalar_scan(op, OFF, rows(T))
    CASES["sc_scan[%s,aidx,exclusive]" % oname] = lambda e, op=op: e.scalar_scan(op, OFF, rows(N_PTS), idx(T, N_PTS), exclusive=True)
CASES["sc_reduce[dot]"] = lambda e: e.scalar_reduce(ZKP_SC_DOT, OFF, rows(T), None, rows(T), None)
CASES["sc_reduce[dot,aidx]"] = lambda e: e.scalar_reduce(ZKP_SC_DOT, OFF, rows(N_PTS), idx(T, N_PTS), rows(T), None)
CASES["sc_reduce[dot,aidx,bidx]"] = lambda e: e.scalar_reduce(ZKP_SC_DOT, OFF, rows(N_PTS), idx(T, N_PTS), rows(3), idx(T, 3))
CASES["sc_reduce[sum,no terms]"] = lambda e: e.scalar_reduce(ZKP_SC_SUM, np.zeros(4, np.uint32), rows(0))
CASES["mul_base"] = lambda e: e.mul_base(rows(N))
for with_pidx in (False, True):
    for with_neg in (False, True):
        tag = ",".join(t for t, on in (("pidx", with_pidx), ("neg", with_neg)) if on)

        def args(with_pidx=with_pidx, with_neg=with_neg):
            return (OFF, rows(N_PTS if with_pidx else T), idx(T, N_PTS) if with_pidx else None, idx(T, 2).astype(np.uint8) if with_neg else None)
        CASES["sum_points[%s]" % tag] = lambda e, args=args: e.sum_points(*args())
        CASES["scan_points[%s]" % tag] = lambda e, args=args: e.point_scan(*args())
CASES["sum_points[no terms]"] = lambda e: e.sum_points(np.zeros(4, np.uint32), rows(N_PTS), np.zeros(0, np.uint32))
CASES["dlog_base"] = _dlog_base
CASES["dlog_point"] = _dlog_point(False)
CASES["dlog_point[signed]"] = _dlog_point(True)
CASES["transcripts_append_message"] = lambda e: e.transcripts_append_message(rows(2, 208), b"label", *MSGS)
CASES["transcripts_append_message[shared]"] = lambda e: e.transcripts_append_message(rows(2, 208), b"label", *MSGS, shared_initial=True)
CASES["transcripts_challenge_bytes"] = lambda e: e.transcripts_challenge_bytes(rows(N, 208), b"label", 33)
CASES["transcripts_challenge_bytes[0]"] = lambda e: e.transcripts_challenge_bytes(rows(N, 208), b"label", 0)
CASES["transcripts_challenge_scalars"] = lambda e: e.transcripts_challenge_scalars(rows(N, 208), b"label")
CASES["transcripts_append_points"] = lambda e: e.transcripts_append_points(rows(N, 208), b"kind", b"var", rows(N))
CASES["transcripts_witness_rng"] = lambda e: e.transcripts_witness_rng(rows(N, 208), b"label", np.zeros((N, 2, 32), np.uint8), rows(N), ZKP_RNG_SCALARS, 3)
CASES["debug_quad_selftest"] = lambda e: e.debug_quad_selftest(rows(N, 64))
CASES["debug_row_selftest"] = lambda e: e.debug_row_selftest(rows(N, 64))

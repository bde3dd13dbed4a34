"""(helper module of tests/test_host_product_history.py and tests/test_gpu_product_history.py)
One seeded, fixed script of calls for ONE long-lived context that runs the batched product calls of include/zkp_mi355x.h sections (5) to (13)
-- hash to group, the scalar calls, the transcript calls and TranscriptRng, mul_base / mul_points, point sums, msm_segments, scalar reduce, the
two scans, dlog_base and dlog_point -- between proof flows, after one another, across a workspace reallocation and with each other's tables
alive.  It continues tests/context_history_cases.py (whose proof, option and register steps it imports, and whose script it leaves alone).

The transitions, in script order (build() names each in a comment):

  f'  ZKP_OPT_WS_LIMIT_BYTES = 1 MiB in front of a product call that needs more: refused, then the limit lifted and the same call correct
  d   growth under live persistent objects: the CMZ common points registered, the first mul_base (the table of B), prepare_dlog(8),
      prepare_dlog_point on slots 0 and 7, a recorded graph of five product calls (GPU only), smaller calls, the graph replayed, then a call
      larger than anything before it -- and every table, slot and registration still gives its catalogue bytes; the graph is stale
  a   every product call once at n = 65 right behind 256 CMZ proofs
  b   the proof flows behind the block of product calls: CMZ prove at N = 64, the three verify flows with planted mutants
  c   every product call at n = 65 followed by a call of each other family at n = 9
  f   a call refused for its arguments between two good ones, per family
  g   the option words the term path behind msm_segments reads (c->batch_encode_min, comb_teeth, grouped_comb, tables_lane,
      ct_single_use_tables, ladder_interleave, comb_split; ct_lookup has one value in this build), flipped between two identical calls and back
  e   ZKP_DLOG_SLOTS + 1 bases through toolbox.point_dlog with a DLEQ verification between every two: the least recently used slot goes

Steps are dicts: kind, the call's inputs, `expect` and `source`.  No expectation comes from the device, none for a product call from the code
under test (the host backend included).  The source per step kind:

  product  from_uniform, hash_from_bytes            "oracle"   oracle.cbind.from_uniform_bytes (of hashlib's digest)
           sc_invert, sc_from_wide, sc_muladd,      "python"   Python integers, hashlib; zkp_chacha20_block through
           sc_hash, sc_random, sc_reduce, sc_scan              tests.test_host_scalar_ops / scalar_reduce_cases / scan_cases
           tr_append, tr_challenge, tr_rng,         "model"    oracle.model's Strobe128 / Transcript / TranscriptRng in Python, started from
           tr_chal_scalars, tr_append_points                   the 208-byte blob
           mul_base, mul_points, msm_segments       "oracle"   oracle.cbind.msm_many (point_mul_cases, msm_segments_cases)
           add_points                               "model"    oracle.model's big integers (point_sum_cases.pair_expected)
           sum_points                               "oracle"   point_sum_cases.segments_expected
           pt_scan                                  "cases"    scan_cases.pt_expected: multiples of B chosen by their logarithms
           dlog_base, dlog_point, dlog_toolbox      "chosen"   the integers k the case modules encoded (dlog_cases, dlog_point_cases)
  prove, msm_many                                   "oracle"   as in context_history_cases
  verify_compact, verify_each, batch                "planted"
  refused                                           "refused"  the status: ZKP_ERR_ARG on an engine, ZKP_TB_BAD_STATEMENT from the toolbox with
                                                               ctx == NULL for the same argument; Oom for the workspace limit (engine only)
  graph_capture, graph_replay                       "model" / "oracle" / "python": the expectations of the direct product steps
  option, register, prepare_dlog, prepare_dlog_point, graph_stale: no result

run_step(eng, s) replays one step on an Engine of either build, or with eng = None on the toolbox with ctx == NULL; check(s, got) compares
byte for byte and names the step.  The GPU-only kinds (graph_*) and the measurements are the GPU test's."""
import hashlib

import numpy as np

from oracle import cbind as C
from oracle import model as M
from tests import context_history_cases as H
from tests import dlog_cases as DC
from tests import dlog_point_cases as PD
from tests import msm_segments_cases as MS
from tests import point_mul_cases as PC
from tests import point_sum_cases as SC
from tests import scalar_reduce_cases as RC
from tests import scan_cases as SCN
from tests import transcript_rng_cases as TR
from tests.scalar_edge_cases import L, VALUES, random_256
from tests.test_host_scalar_ops import WIDE_EDGES, chacha_block, muladd_operands, rows, want_hash

SEED = 20261020
N_BIG, N_SMALL = 65, 9
FAMILIES = {"hash": ("from_uniform", "hash_from_bytes"),
            "scalar": ("sc_invert", "sc_from_wide", "sc_muladd", "sc_hash", "sc_random"),
            "transcript": ("tr_append", "tr_challenge", "tr_rng", "tr_chal_scalars", "tr_append_points"),
            "pairwise": ("mul_base", "mul_points", "add_points"),
            "fold": ("sum_points", "msm_segments", "sc_reduce"),
            "scan": ("sc_scan", "pt_scan"),
            "dlog": ("dlog_base", "dlog_point")}
FAMILY_OF = {c: f for f, calls in FAMILIES.items() for c in calls}
CALLS = tuple(c for calls in FAMILIES.values() for c in calls)
OPT = dict(BATCH_ENCODE_MIN=1, COMB_TEETH=2, CT_SINGLE_USE_TABLES=3, GROUPED_COMB=6, TABLES_LANE=7, LADDER_INTERLEAVE=11, WS_LIMIT_BYTES=12, COMB_SPLIT=16)
DEFAULT = H.DEFAULT
KEY, NONCE = bytes(range(7, 39)), 0x0badc0de12345678
DLOG_BABY, DLOG_BITS = 8, 16
SLOTS = {0: ("G7", 4), 7: ("H", 8)}                    # slot -> (base of dlog_point_cases, baby_bits)
DLOG_POINT_BITS = 12
GRAPH_CALLS = ("mul_points", "sc_scan", "tr_append_points", "tr_rng", "tr_chal_scalars")
Oom = H.Oom
REFUSED = "refused"
_CACHE = {}


# ---- transcripts: the 208-byte blob <-> oracle.model --------------------------------------------------------------------------------------------
def model_of(blob):
    """oracle.model.Transcript standing where the blob stands: 200 bytes of state, then pos, pos_begin, cur_flags"""
    s = object.__new__(M.Strobe128)
    s.state = bytearray(bytes(blob[:200]))
    s.pos, s.pos_begin, s.cur_flags = int(blob[200]), int(blob[201]), int(blob[202])
    t = object.__new__(M.Transcript)
    t.strobe = s
    return t


def blob_of(t, like):
    """the blob of a model transcript; bytes 203 .. 207 (padding) as in `like`"""
    b = np.array(like, np.uint8, copy=True)
    b[:200] = np.frombuffer(bytes(t.strobe.state), np.uint8)
    b[200:203] = (t.strobe.pos, t.strobe.pos_begin, t.strobe.cur_flags)
    return b


def states(n, shift=0):
    """n start states of transcript_ops_cases at a mix of positions; row 0 stands at position 165"""
    S = TR.start_states()
    idx = [(37 * j + shift) % len(S) for j in range(n)]
    idx[0] = TR.state_at(165)
    return np.ascontiguousarray(S[idx])


def model_append(ts, label, msgs):
    out = []
    for b, m in zip(ts, msgs):
        t = model_of(b)
        t.append_message(label, bytes(m))
        out.append(blob_of(t, b))
    return np.stack(out)


def model_challenge(ts, label, n_bytes):
    out, adv = [], []
    for b in ts:
        t = model_of(b)
        out.append(np.frombuffer(t.challenge_bytes(label, n_bytes), np.uint8))
        adv.append(blob_of(t, b))
    return np.stack(out).reshape(len(ts), n_bytes), np.stack(adv)


def model_rng(ts, label, wit, ent, mode, count):
    out = []
    for b, w, e in zip(ts, wit, ent):
        r = model_of(b).build_rng()
        for k in range(w.shape[0]):
            r = r.rekey_with_witness_bytes(label, w[k].tobytes())
        rng = r.finalize(e.tobytes())
        if mode == 0:
            out.append(np.frombuffer(b"".join(M.sc_to_bytes(rng.random_scalar()) for _ in range(count)), np.uint8).reshape(count, 32))
        else:
            out.append(np.frombuffer(rng.fill_bytes(count), np.uint8))
    return np.stack(out)


def model_challenge_scalars(ts, label):
    wide, adv = model_challenge(ts, label, 64)
    return rows([int.from_bytes(w.tobytes(), "little") % L for w in wide]), adv


def model_append_points(ts, kind, label, pts, validate):
    st, out = np.zeros(len(ts), np.uint8), []
    for j, (b, p) in enumerate(zip(ts, pts)):
        if validate and not p.any():
            st[j] = 1
            out.append(np.array(b, np.uint8, copy=True))
            continue
        t = model_of(b)
        t.append_message(kind, label)
        t.append_message(b"val", p.tobytes())
        out.append(blob_of(t, b))
    return st, np.stack(out)


# ---- one product call at size n: inputs and expectation, built once per (call, n) ---------------------------------------------------------------
def _lens(n, long_one=True):
    """n segment lengths: empty, short and medium ones in turn, and (n >= 65) one of 300 terms in the middle"""
    lens = [(1, 2, 0, 7, 40, 3)[i % 6] for i in range(n)]
    if long_one and n >= N_BIG:
        lens[n // 2] = 300
    return lens


def chunk():
    from zkp_amd import toolbox as T
    return int(T.lib().zkp_dlog_chunk())


def _messages(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.bytes((0, 1, 111, 112, 127, 128, 239, 240, 60)[j % 9]) for j in range(n)]


def _make(call, n, lens=None):
    rng = np.random.default_rng([SEED, CALLS.index(call), n])
    s = dict(kind="product", call=call, family=FAMILY_OF[call], n=n, name="%s n=%d" % (call, n))
    if call == "from_uniform":
        inp = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        s.update(inp=inp, expect=PC.enc_rows([C.from_uniform_bytes(r.tobytes()) for r in inp]), source="oracle")
    elif call == "hash_from_bytes":
        msgs = _messages(n, n + 1)
        s.update(msgs=msgs, expect=PC.enc_rows([C.from_uniform_bytes(hashlib.sha512(m).digest()) for m in msgs]), source="oracle")
    elif call == "sc_invert":
        vals = ([0, 1, L - 1, L, L + 1, 2**256 - 1] + VALUES[n % 40:n % 40 + 30] + random_256(n, n))[:n]
        s.update(a=rows(vals), expect=rows([pow(v % L, L - 2, L) for v in vals]), source="python")
    elif call == "sc_from_wide":
        vals = (WIDE_EDGES + [int.from_bytes(rng.bytes(64), "little") for _ in range(n)])[:n]
        s.update(a=rows(vals, 64), expect=rows([v % L for v in vals]), source="python")
    elif call == "sc_muladd":
        recs = muladd_operands()[3 * n:4 * n]
        s.update(a=rows([r[0] for r in recs]), b=rows([r[1] for r in recs]), c=rows([r[2] for r in recs]),
                 expect=rows([(a * b + c) % L for a, b, c in recs]), source="python")
    elif call == "sc_hash":
        msgs = _messages(n, n + 2)
        s.update(msgs=msgs, expect=rows(want_hash(msgs)), source="python")
    elif call == "sc_random":
        s.update(expect=rows([int.from_bytes(chacha_block(KEY, i, NONCE + n), "little") % L for i in range(n)]), source="python")
    elif call == "tr_append":
        ts = states(n, 1)
        msgs = [bytes(rng.integers(0, 256, size=(0, 60, 167, 5, 166)[j % 5], dtype=np.uint8)) for j in range(n)]
        s.update(ts=ts, label=b"msg", msgs=msgs, expect=model_append(ts, b"msg", msgs), source="model")
    elif call == "tr_challenge":
        ts = states(n, 2)
        s.update(ts=ts, label=b"chal", n_bytes=200, expect=model_challenge(ts, b"chal", 200), source="model")
    elif call == "tr_rng":
        ts = states(n, 3)
        wit, ent = rng.integers(0, 256, size=(n, 2, 32), dtype=np.uint8), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        mode, count = (0, 2) if n >= N_BIG else (1, 64)
        s.update(ts=ts, label=b"w", wit=wit, ent=ent, mode=mode, count=count, expect=model_rng(ts, b"w", wit, ent, mode, count), source="model")
    elif call == "tr_chal_scalars":
        ts = states(n, 4)
        s.update(ts=ts, label=b"chal", expect=model_challenge_scalars(ts, b"chal"), source="model")
    elif call == "tr_append_points":
        ts = states(n, 5)
        pts = TR.points(n, [1, n - 1] if n > 2 else [])
        s.update(ts=ts, kind_label=b"ptvar", label=b"A", pts=pts, expect=model_append_points(ts, b"ptvar", b"A", pts, True), source="model")
    elif call == "mul_base":
        k = (7 * n) % 50
        s.update(sc=PC.base_operands()[k:k + n].copy(), expect=PC.base_expected()[k:k + n].copy(), source="oracle")
    elif call == "mul_points":
        sc, pt, _ = PC.pair_operands()
        out, st = PC.pair_expected()
        k = len(sc) - n                                                          # the tail: the invalid encodings between valid neighbours
        s.update(sc=sc[k:].copy(), pts=pt[k:].copy(), expect=(out[k:].copy(), st[k:].astype(np.uint8)), source="oracle")
    elif call == "add_points":
        a, b, _ = SC.pair_operands()
        out, st = SC.pair_expected(SC.ADD)
        s.update(a=a[:n].copy(), b=b[:n].copy(), expect=(out[:n].copy(), st[:n].copy()), source="model")
    elif call == "sum_points":
        off = RC.offsets(_lens(n))
        pts, bad = SC.catalogue()
        t = int(off[-1])
        pidx = rng.integers(0, len(pts) - 1, size=t)
        pidx[pidx >= bad] += 1
        if n > 4:
            pidx[int(off[4])] = bad                                              # one sum references the row that does not decode
        neg = (rng.integers(0, 3, size=t) == 0).astype(np.uint8)
        pidx = pidx.astype(np.uint32)
        out, st = SC.segments_expected(off, pidx, neg, pts)
        s.update(off=off, pts=pts, pidx=pidx, neg=neg, expect=(out, st.astype(np.uint8)), source="oracle")
    elif call == "msm_segments":
        off, sc, pidx, pts = MS.job(lens if lens is not None else _lens(n), seed=n)
        flags = 1 if lens is not None else 0
        out, st = C.msm_many(off, sc, pidx, pts, flags)
        s.update(off=off, sc=sc, pidx=pidx, pts=pts, flags=flags, expect=(out, st), source="oracle")
    elif call == "sc_reduce":
        op = RC.DOT
        _, off, a, _, b, _ = RC.job(op, _lens(n), seed=n)
        s.update(op=op, off=off, a=RC.rows(a), b=RC.rows(b), expect=RC.rows(RC.expected(op, off, a, None, b, None)), source="python")
    elif call == "sc_scan":
        op = SCN.PRODUCT if lens is None else SCN.SUM
        _, off, a, _ = SCN.sc_job(op, lens if lens is not None else _lens(n), seed=n)
        s.update(op=op, off=off, a=RC.rows(a), exclusive=False, expect=RC.rows(SCN.sc_expected(op, off, a)), source="python")
    elif call == "pt_scan":
        ln = _lens(n)
        off, pidx, neg = SCN.pt_job(ln, seed=n, bad_at=(int(sum(ln[:5])),) if n > 5 else ())
        out, st = SCN.pt_expected(off, pidx, neg, False)
        s.update(off=off, pts=SCN.catalogue(), pidx=pidx, neg=neg, expect=(out, st), source="cases")
    elif call == "dlog_base":
        pts, k, st = DC.tiled(DLOG_BABY, DLOG_BITS, chunk(), n)
        s.update(pts=pts, bits=DLOG_BITS, expect=(k, st), source="chosen")
    elif call == "dlog_point":
        return dlog_point_step(0, n, False)
    else:
        raise ValueError(call)
    return s


def product_step(call, n, lens=None):
    key = (call, n, None if lens is None else tuple(lens))
    if key not in _CACHE:
        _CACHE[key] = _make(call, n, lens)
    return _CACHE[key]


def dlog_point_step(slot, n, signed):
    key = ("dlog_point", slot, n, signed)
    if key not in _CACHE:
        name, bb = SLOTS[slot]
        pts, k, st = PD.tiled(name, bb, DLOG_POINT_BITS, chunk(), n, signed)
        _CACHE[key] = dict(kind="product", call="dlog_point", family="dlog", n=n, name="dlog_point slot %d (%s) n=%d%s" % (slot, name, n, " signed" if signed else ""),
                           slot=slot, base=PD.base(name), baby_bits=bb, pts=pts, bits=DLOG_POINT_BITS, signed=signed, expect=(k, st), source="chosen")
    return _CACHE[key]


def refused_step(family):
    """a call of the family with an argument its own test_argument_errors_* list holds: ZKP_ERR_ARG, nothing launched"""
    return dict(kind="refused", family=family, how="arg", name="refused %s call" % family, expect=REFUSED, source="refused")


def option_step(name, value, refused=False):
    return dict(kind="option", option=OPT[name], name=name, value=value, refused=refused)


def graph_expect():
    """what the recorded chain leaves behind, from the expectations of the direct steps: mul_points, sc_scan, then on the transcripts of
    tr_append_points: the appends, the witness RNG over the appended transcripts, get_challenge"""
    if "graph" not in _CACHE:
        mp, scan, ap, rg = (product_step(c, N_BIG) for c in GRAPH_CALLS[:4])
        st, ts1 = ap["expect"]
        nonce = model_rng(ts1, rg["label"], rg["wit"], rg["ent"], 0, 2)
        chal, ts2 = model_challenge_scalars(ts1, b"chal")
        _CACHE["graph"] = dict(mul=mp["expect"], scan=scan["expect"], status=st, nonce=nonce, chal=chal, ts=ts2)
    return _CACHE["graph"]


def dlog_toolbox_steps():
    """ZKP_DLOG_SLOTS + 1 distinct bases and the first one again: (100 + i) B for i < 6, then B, G7 and H"""
    ks = [0, 1, 5, 77, (1 << DLOG_POINT_BITS) - 1]
    out = []
    others = PD.other_bases(6)
    for i, base in enumerate(others):
        pts = DC.encode_multiples([k * (100 + i) for k in ks])
        out.append((base, pts))
    for name in PD.BASES:
        out.append((PD.base(name), PD.encode_multiples(name, ks)))
    assert len({b for b, _ in out}) == 9
    out.append(out[0])
    return [dict(kind="dlog_toolbox", base=b, pts=p, bits=DLOG_POINT_BITS, name="toolbox.point_dlog base %d" % (i % 9), again=i == 9,
                 expect=(np.array(ks, np.uint64), np.zeros(len(ks), np.uint8)), source="chosen") for i, (b, p) in enumerate(out)]


OOM_LENS = (20000, 19999, 1)                             # 40,000 scalars: 1.28 MB in, 1.28 MB out
BIG_MSM_LENS = (600, 0, 300, 1, 200, 37)                  # 1,138 constant-time terms: the classified term path behind msm_segments


def build():
    """-> the list of steps (built once per process)"""
    if "script" in _CACHE:
        return _CACHE["script"]
    rng = np.random.default_rng(SEED)
    S = []
    cmz_big, cmz_mid = H._proofs("cmz", 256, rng), H._proofs("cmz", 64, rng)
    dleq = {n: H._proofs("dleq", n, rng) for n in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)}
    common = cmz_mid["common"]
    P = product_step

    # ---- f'. the workspace limit in front of a product call that needs more (before anything large: the limit refuses growth) ---------------
    S.append(P("sc_invert", N_SMALL))
    S.append(option_step("WS_LIMIT_BYTES", 1 << 20))
    S.append(dict(P("sc_scan", 3, OOM_LENS), oom=True))
    S.append(P("sc_invert", N_SMALL))
    S.append(option_step("WS_LIMIT_BYTES", 0))
    S.append(P("sc_scan", 3, OOM_LENS))

    # ---- d. growth under live persistent objects ----------------------------------------------------------------------------------------------
    S.append(dict(kind="register", encodings=np.ascontiguousarray(common)))
    S.append(dict(P("mul_base", N_SMALL), first_mul_base=True))                  # builds the table of B
    S.append(dict(kind="prepare_dlog", baby_bits=DLOG_BABY))
    for slot, (name, bb) in SLOTS.items():
        S.append(dict(kind="prepare_dlog_point", slot=slot, base=PD.base(name), baby_bits=bb))
    for c in GRAPH_CALLS:
        S.append(P(c, N_BIG))                                                    # the direct calls whose _dev forms the graph records
    S.append(dict(kind="graph_capture", source="model"))                         # (GPU only)
    for c in GRAPH_CALLS:
        S.append(P(c, N_SMALL))                                                  # other calls that do not grow the workspace
    S.append(dict(kind="graph_replay", source="model"))                          # (GPU only)
    S.append(dict(H.prove_step(cmz_big), grows=True))                            # larger than anything before it: ensure_ws reallocates
    S.append(dict(P("dlog_base", N_BIG), after_growth=True))
    for slot in SLOTS:
        for signed in (False, True):
            S.append(dict(dlog_point_step(slot, N_BIG, signed), after_growth=True))
    S.append(dict(P("mul_base", N_BIG), after_growth=True))
    S.append(dict(H.msm_step(common, None, np.random.default_rng(3), 1), after_growth=True))
    S.append(dict(H.prove_step(cmz_mid), after_growth=True))
    S.append(dict(kind="graph_stale"))                                           # (GPU only)

    # ---- a. every product call at n = 65 behind the large proof flow --------------------------------------------------------------------------
    S.append(H.prove_step(cmz_big))
    for c in CALLS:
        S.append(dict(P(c, N_BIG), measure=True))

    # ---- b. the proof flows behind the block of product calls ---------------------------------------------------------------------------------
    S.append(dict(H.prove_step(cmz_mid), after_products=True))
    S.append(H.verify_step("verify_compact", cmz_mid, {0, 31, 63}, rng))
    S.append(H.verify_step("verify_each", cmz_mid, {1, 62}, rng))
    S.append(H.verify_step("batch", cmz_mid, {40}, rng, K=2))

    # ---- c. every product call at n = 65, then a call of each other family at n = 9 ----------------------------------------------------------
    turn = {f: 0 for f in FAMILIES}
    for c in CALLS:
        for f, calls in FAMILIES.items():
            if f == FAMILY_OF[c]:
                continue
            S.append(dict(P(c, N_BIG), pair=(c, f)))
            S.append(P(calls[turn[f] % len(calls)], N_SMALL))
            turn[f] += 1

    # ---- f. a refused call between two good ones, per family ----------------------------------------------------------------------------------
    for f in ("scalar", "transcript", "pairwise", "fold", "scan", "dlog"):
        S.append(P(FAMILIES[f][0], N_BIG))
        S.append(refused_step(f))
        S.append(P(FAMILIES[f][-1], N_BIG))

    # ---- g. the option words the launchers behind msm_segments read (1,138 constant-time terms: classified), flipped and flipped back --------
    probe = P("msm_segments", len(BIG_MSM_LENS), BIG_MSM_LENS)
    S.append(probe)
    for name, values, refused in (("BATCH_ENCODE_MIN", (0, 65536), ()), ("COMB_TEETH", (16, 8, 4), (8,)), ("GROUPED_COMB", (1, 0, DEFAULT), ()),
                                  ("TABLES_LANE", (1, 0, DEFAULT), ()), ("CT_SINGLE_USE_TABLES", (1, 0, DEFAULT), ()), ("LADDER_INTERLEAVE", (1, 0, DEFAULT), ()),
                                  ("COMB_SPLIT", (1, 0, DEFAULT), ())):
        for v in values:
            S.append(option_step(name, v, refused=v in refused))
            S.append(probe)

    # ---- e. dlog slots replaced between proofs, through the toolbox ---------------------------------------------------------------------------
    for i, s in enumerate(dlog_toolbox_steps()):
        S.append(s)
        S.append(H.verify_step("verify_compact", dleq[5 + i], {0} if i % 2 else set(), rng))
    _CACHE["script"] = S
    return S


# ---- replay -------------------------------------------------------------------------------------------------------------------------------------
def _refused_call(eng, family):
    """the refused call of a family on an engine -> REFUSED when the library said ZKP_ERR_ARG"""
    from zkp_amd.engine import ZkpError
    p = product_step(FAMILIES[family][0], N_BIG)
    try:
        if family == "scalar":
            m = product_step("sc_muladd", N_BIG)
            out = np.zeros((N_BIG, 32), np.uint8)
            ptr = lambda a: a.ctypes.data
            rc = eng._lib.zkp_sc_muladd(eng._h, N_BIG, ptr(m["a"]), 2, ptr(m["b"]), 1, ptr(m["c"]), 1, ptr(out))       # strides must be 0 or 1
            assert not out.any()
            return REFUSED if rc == -2 else rc
        if family == "transcript":
            t = product_step("tr_chal_scalars", N_BIG)
            ts = t["ts"].copy()
            try:
                eng.transcripts_challenge_scalars(ts, 249 * b"x")                # a label longer than 248 bytes
            finally:
                assert (ts == t["ts"]).all()
        elif family == "pairwise":
            m = product_step("mul_points", N_BIG)
            eng.mul_points(m["sc"], m["pts"], 7)                                 # flags: neither ZKP_CT nor ZKP_VARTIME
        elif family == "fold":
            m = product_step("msm_segments", N_BIG)
            eng.msm_segments(m["off"], m["sc"], m["pts"], m["pidx"], 7)
        elif family == "scan":
            m = product_step("sc_scan", N_BIG)
            eng.scalar_scan(7, m["off"], m["a"])                                 # op: neither ZKP_SC_SUM nor ZKP_SC_PRODUCT
        elif family == "dlog":
            eng.dlog_base(p["pts"], 49)                                          # bits must be 1 .. 48
        else:
            raise ValueError(family)
    except ZkpError as e:
        return REFUSED if "code -2:" in str(e) else str(e)
    return "accepted"


def _refused_host(family):
    """the same bad argument through the toolbox with ctx == NULL -> REFUSED when it said ZKP_TB_BAD_STATEMENT (-10) and wrote nothing"""
    from zkp_amd import toolbox as T
    from zkp_amd.engine import ZkpError
    try:
        if family == "scalar":
            m = product_step("sc_muladd", N_BIG)
            out = np.zeros((N_BIG, 32), np.uint8)
            rc = T.lib().zkp_scalar_muladd_batch(None, N_BIG, T._p(m["a"]), 2, T._p(m["b"]), 1, T._p(m["c"]), 1, 0, T._p(out))
            assert not out.any()
            return REFUSED if rc == -10 else rc
        if family == "transcript":
            t = product_step("tr_chal_scalars", N_BIG)
            ts = t["ts"].copy()
            try:
                T.challenge_scalars(None, ts, 249 * b"x")
            finally:
                assert (ts == t["ts"]).all()
        elif family == "pairwise":
            m = product_step("mul_points", N_BIG)
            T.point_mul(None, m["sc"], m["pts"], 7)
        elif family == "fold":
            m = product_step("msm_segments", N_BIG)
            T.multiscalar_sum(None, m["off"], m["sc"], m["pts"], m["pidx"], 7)
        elif family == "scan":
            m = product_step("sc_scan", N_BIG)
            T.scalar_scan(None, 7, m["off"], m["a"])
        elif family == "dlog":
            T.basepoint_dlog(None, product_step("dlog_base", N_BIG)["pts"], 49)
        else:
            raise ValueError(family)
    except ZkpError as e:
        return REFUSED if "code -10:" in str(e) else str(e)
    return "accepted"


def _product(eng, s):
    from zkp_amd import toolbox as T
    call = s["call"]
    if call == "from_uniform":
        return eng.from_uniform_bytes(s["inp"]) if eng else T.from_uniform_bytes(None, s["inp"])
    if call == "hash_from_bytes":
        return eng.hash_from_bytes_sha512(s["msgs"]) if eng else T.hash_from_bytes_sha512(None, s["msgs"])
    if call == "sc_invert":
        return eng.scalar_invert(s["a"]) if eng else T.scalar_invert(None, s["a"])
    if call == "sc_from_wide":
        return eng.scalar_from_wide(s["a"]) if eng else T.scalar_from_wide(None, s["a"])
    if call == "sc_muladd":
        return eng.scalar_muladd(s["a"], s["b"], s["c"]) if eng else T.scalar_muladd(None, s["a"], s["b"], s["c"])
    if call == "sc_hash":
        return eng.scalar_hash_from_bytes_sha512(s["msgs"]) if eng else T.scalar_hash_from_bytes_sha512(None, s["msgs"])
    if call == "sc_random":
        return eng.scalar_random(s["n"], KEY, NONCE + s["n"]) if eng else T.scalar_random(None, s["n"], KEY, NONCE + s["n"])
    if call.startswith("tr_"):
        ts = s["ts"].copy()
        if call == "tr_append":
            from zkp_amd.engine import messages_csr
            data, offsets = messages_csr(s["msgs"])
            return eng.transcripts_append_message(ts, s["label"], data, offsets) if eng else T.append_messages_csr(ts, s["label"], data, offsets)
        if call == "tr_challenge":
            out = eng.transcripts_challenge_bytes(ts, s["label"], s["n_bytes"]) if eng else T.challenge_bytes(None, ts, s["label"], s["n_bytes"])
            return out, ts
        if call == "tr_rng":
            if eng:
                out = eng.transcripts_witness_rng(ts, s["label"], s["wit"], s["ent"], s["mode"], s["count"])
            else:
                out = (T.witness_rng_bytes if s["mode"] else T.witness_rng_scalars)(None, ts, s["wit"], s["count"], s["ent"], s["label"])
            assert (ts == s["ts"]).all(), "the witness RNG changed its transcripts"
            return out
        if call == "tr_chal_scalars":
            out = eng.transcripts_challenge_scalars(ts, s["label"]) if eng else T.challenge_scalars(None, ts, s["label"])
            return out, ts
        st = eng.transcripts_append_points(ts, s["kind_label"], s["label"], s["pts"], True) if eng else T.append_point_vars(None, ts, s["label"], s["pts"], True)
        return st, ts
    if call == "mul_base":
        return eng.mul_base(s["sc"]) if eng else T.basepoint_mul(None, s["sc"])
    if call == "mul_points":
        return eng.mul_points(s["sc"], s["pts"], 1) if eng else T.point_mul(None, s["sc"], s["pts"], 1)
    if call == "add_points":
        return eng.add_points(s["a"], s["b"], 0) if eng else T.point_add(None, s["a"], s["b"])
    if call == "sum_points":
        return eng.sum_points(s["off"], s["pts"], s["pidx"], s["neg"]) if eng else T.point_sum(None, s["off"], s["pts"], s["pidx"], s["neg"])
    if call == "msm_segments":
        if eng:
            return eng.msm_segments(s["off"], s["sc"], s["pts"], s["pidx"], s["flags"])
        return T.multiscalar_sum(None, s["off"], s["sc"], s["pts"], s["pidx"], s["flags"])
    if call == "sc_reduce":
        return eng.scalar_reduce(s["op"], s["off"], s["a"], None, s["b"], None) if eng else T.scalar_reduce(None, s["op"], s["off"], s["a"], None, s["b"], None)
    if call == "sc_scan":
        return eng.scalar_scan(s["op"], s["off"], s["a"], None, s["exclusive"]) if eng else T.scalar_scan(None, s["op"], s["off"], s["a"], None, s["exclusive"])
    if call == "pt_scan":
        return eng.point_scan(s["off"], s["pts"], s["pidx"], s["neg"], False) if eng else T.point_cumsum(None, s["off"], s["pts"], s["pidx"], s["neg"], False)
    if call == "dlog_base":
        if eng is None:
            return T.basepoint_dlog(None, s["pts"], s["bits"])
        if eng.dlog_baby_bits != DLOG_BABY:                                      # (a context used for this call alone: the measurement of part a; the GPU replay
                                                                                 #  asserts that the long-lived context never comes here after step d)
            eng.prepare_dlog(DLOG_BABY)
        return eng.dlog_base(s["pts"], s["bits"])
    if call == "dlog_point":
        if eng is None:
            return T.point_dlog(None, s["base"], s["pts"], s["bits"], s["signed"])
        if eng.dlog_point_slots()[s["slot"]] != (bytes(s["base"]), s["baby_bits"]):
            eng.prepare_dlog_point(s["slot"], s["base"], s["baby_bits"])
        return eng.dlog_point(s["slot"], s["pts"], s["bits"], s["signed"])
    raise ValueError(call)


def run_step(eng, s):
    """one step on `eng` (an Engine of either build; None = the toolbox with ctx == NULL) -> what the call returned, in the form of s["expect"]
    (None for steps without a result, Oom for a call the workspace limit refused).  The graph steps are the GPU test's."""
    from zkp_amd import toolbox as T
    kind = s["kind"]
    if kind == "product":
        if s.get("oom") and eng is not None:                                     # the raw call: the output rows must stay as they were
            assert s["call"] == "sc_scan"
            out = np.full((int(s["off"][-1]), 32), 0x5a, np.uint8)
            ptr = lambda a: a.ctypes.data
            rc = eng._lib.zkp_sc_scan(eng._h, s["op"], 0, len(s["off"]) - 1, ptr(s["off"]), ptr(s["a"]), len(s["a"]), None, ptr(out))
            assert (out == 0x5a).all(), "a refused call wrote to its output"
            return Oom if rc == -4 else rc                                       # ZKP_ERR_OOM
        try:
            return _product(eng, s)
        except Exception as e:
            if s.get("oom") and "code -4:" in str(e):                            # ZKP_ERR_OOM
                return Oom
            raise
    if kind == "refused":
        return _refused_host(s["family"]) if eng is None else _refused_call(eng, s["family"])
    if kind == "prepare_dlog":
        if eng is not None:
            eng.prepare_dlog(s["baby_bits"])
        return None
    if kind == "prepare_dlog_point":
        if eng is not None:
            eng.prepare_dlog_point(s["slot"], s["base"], s["baby_bits"])
        return None
    if kind == "dlog_toolbox":
        before = T.get_dlog_host_max_steps()
        T.set_dlog_host_max_steps(0)                                             # the device route, whatever the size
        try:
            return T.point_dlog(eng, s["base"], s["pts"], s["bits"])
        finally:
            T.set_dlog_host_max_steps(before)
    return H.run_step(eng, s)


def check(s, got):
    """got == s["expect"], byte for byte; the assertion names the step"""
    exp = s["expect"]
    name = s.get("name") or "%s%s" % (s["kind"], " N=%d %s" % (s["n"], s["which"]) if "which" in s else "")
    if isinstance(exp, str) or exp is Oom:
        assert got == exp or got is exp, "%s: %r instead of %r" % (name, got, exp)
        return
    exp, got = (exp, got) if isinstance(exp, tuple) else ((exp,), (got,))
    assert len(got) == len(exp), name
    for i, (a, e) in enumerate(zip(got, exp)):
        a, e = np.asarray(a), np.asarray(e)
        assert a.shape == e.shape, "%s: result %d has shape %s, expected %s" % (name, i, a.shape, e.shape)
        if not np.array_equal(a, e):
            bad = np.flatnonzero((a != e).reshape(len(e), -1).any(axis=1))
            raise AssertionError("%s (source: %s): result %d differs in rows %s" % (name, s.get("source"), i, bad[:8].tolist()))

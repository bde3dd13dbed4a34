"""One long-lived context through the script of tests/product_history_cases.py, on the shipped library and on the test-hook build: after EVERY
step the call's bytes are what the catalogue says (C oracle, oracle.model, Python integers, chosen logarithms, planted verdicts -- never the
device, never the host backend), whatever the context went through before.  Held here, besides the replay:

* the GPU-only steps: a graph of mul_points_dev, scalar_scan_dev, transcripts_append_points_dev, transcripts_witness_rng_dev and
  transcripts_challenge_scalars_dev on torch buffers is recorded with the table of B, the context's dlog table, two dlog_point slots and the
  registered points alive, replays to the catalogue's bytes behind other calls, and is refused as stale -- without running -- once a larger
  call has reallocated the workspace;
* (test-hook build) zkp_debug_ws_bytes: the growing call really grows the workspace; every product call at n = 65 behind 256 CMZ proofs runs
  in a workspace at least 8 times what it asks for on a fresh context, and does not grow it; the call the workspace limit refuses allocates
  nothing;
* (shipped build: the toolbox takes contexts of the shipped library only) toolbox.point_dlog over nine bases replaces a free slot first and
  then the slot with the smallest zkp_dlog_point_last_use, the slots prepared by hand included; the first base is built again.

After every step the context's streams are synchronised; an error there ends the session: nothing further is launched on that card."""
import numpy as np
import pytest

from tests import product_history_cases as PH

pytestmark = pytest.mark.gpu
ZKP_ERR_ARG = -2
RATIOS = {}                                     # call -> (workspace behind the large call, need on a fresh context): printed with -s


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


def _nothing_runs_after_a_gpu_error(eng, where):
    """a call that faulted leaves its context in error: the session ends there instead of launching the remaining steps on that card"""
    try:
        eng.synchronize()
    except Exception as e:                                   # noqa: BLE001 -- whatever the runtime reports
        pytest.exit("the context reports a GPU error after %s; nothing further is started: %s" % (where, e), returncode=3)


class _Chain:
    """the five product calls of the recorded graph on device buffers, at n = 65: inputs of the script's direct steps"""

    def __init__(self, eng):
        torch = _torch()
        self.eng, self.torch = eng, torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
        self.mp, self.scan, self.ap, self.rg = (PH.product_step(c, PH.N_BIG) for c in PH.GRAPH_CALLS[:4])
        n = PH.N_BIG
        self.n, self.n_terms = n, int(self.scan["off"][-1])
        self.d_sc, self.d_pts, self.d_mul, self.d_mul_st = dev(self.mp["sc"]), dev(self.mp["pts"]), z(n, 32), z(n)
        self.d_off, self.d_a, self.d_scan = dev(self.scan["off"].view(np.int32)), dev(self.scan["a"]), z(self.n_terms, 32)
        self.d_ts0, self.d_ts, self.d_app, self.d_app_st = dev(self.ap["ts"]), z(n, 208), dev(self.ap["pts"]), z(n)
        self.d_wit, self.d_ent, self.d_nonce, self.d_chal = dev(self.rg["wit"]), dev(self.rg["ent"]), z(n, 2, 32), z(n, 32)
        self.outs = (self.d_mul, self.d_mul_st, self.d_scan, self.d_app_st, self.d_nonce, self.d_chal)

    def reset(self):
        for t in self.outs:
            t.fill_(9)
        self.d_ts.copy_(self.d_ts0)
        self.torch.cuda.synchronize()

    def enqueue(self):
        e, n = self.eng, self.n
        ptr = lambda t: t.data_ptr()
        e.mul_points_dev(n, ptr(self.d_sc), 1, ptr(self.d_pts), 1, 1, ptr(self.d_mul), ptr(self.d_mul_st))
        e.scalar_scan_dev(self.scan["op"], 0, len(self.scan["off"]) - 1, ptr(self.d_off), ptr(self.d_a), self.n_terms, None, self.n_terms, ptr(self.d_scan))
        e.transcripts_append_points_dev(n, ptr(self.d_ts), b"ptvar", b"A", ptr(self.d_app), True, ptr(self.d_app_st))
        e.transcripts_witness_rng_dev(n, ptr(self.d_ts), b"w", 2, 32, ptr(self.d_wit), ptr(self.d_ent), 0, 2, ptr(self.d_nonce))
        e.transcripts_challenge_scalars_dev(n, ptr(self.d_ts), b"chal", ptr(self.d_chal))

    def read_and_check(self, where):
        self.eng.synchronize()
        g = PH.graph_expect()
        got = [t.cpu().numpy() for t in self.outs + (self.d_ts,)]
        want = (g["mul"][0], g["mul"][1], g["scan"], g["status"], g["nonce"], g["chal"], g["ts"])
        for name, a, w in zip(("mul_points", "mul_points status", "sc_scan", "append_points status", "witness_rng", "challenge_scalars", "transcripts"), got, want):
            assert np.array_equal(a, np.asarray(w)), "%s: %s differs from the catalogue" % (where, name)


def _slots(eng):
    lib = eng._lib
    return [(int(lib.zkp_dlog_point_baby_bits(eng._h, k)), int(lib.zkp_dlog_point_last_use(eng._h, k))) for k in range(8)]


def _find(eng, base):
    b = np.frombuffer(bytes(base), np.uint8).copy()
    return int(eng._lib.zkp_dlog_point_find(eng._h, b.ctypes.data))


def _replay(eng, hooks):
    from zkp_amd.engine import Engine
    S = PH.build()
    state = {"graph": None, "chain": None, "first_base_built": 0}
    for i, s in enumerate(S):
        kind = s["kind"]
        where = "step %d (%s)" % (i, s.get("name") or kind)
        if kind == "graph_capture":
            ch = _Chain(eng)
            ch.reset()
            ch.enqueue()
            ch.read_and_check(where + ", direct calls")
            ch.reset()
            with eng.capture() as cap:
                ch.enqueue()
            eng.synchronize()
            ch.reset()
            cap.graph.launch()
            ch.read_and_check(where + ", first replay")
            state["graph"], state["chain"] = cap.graph, ch
        elif kind == "graph_replay":
            ch = state["chain"]
            ch.reset()
            state["graph"].launch()
            ch.read_and_check(where)
        elif kind == "graph_stale":
            ch, g = state["chain"], state["graph"]
            ch.reset()
            rc = eng._lib.zkp_graph_launch(g._h, eng._h)
            assert rc == ZKP_ERR_ARG and "workspace was reallocated" in eng._lib.zkp_last_error().decode(), where
            eng.synchronize()
            assert all(bool((t == 9).all().item()) for t in ch.outs), where + ": the stale graph ran"
            g.close()
        elif kind == "dlog_toolbox":
            if hooks:                                        # (the toolbox takes contexts of the shipped library only)
                continue
            before, had = _slots(eng), _find(eng, s["base"])
            got = PH.run_step(eng, s)
            PH.check(s, got)
            now = _find(eng, s["base"])
            assert now >= 0, where
            if had < 0:
                free = [k for k, (bb, _) in enumerate(before) if bb == 0]
                if free:
                    assert now in free, (where, before, now)
                else:                                        # no slot is free: the least recently used one goes, prepared by hand or not
                    assert before[now][1] == min(u for _, u in before), (where, before, now)
                state["first_base_built"] += bool(s.get("again") or bytes(s["base"]) == bytes(PH.dlog_toolbox_steps()[0]["base"]))
            else:
                assert now == had, where
            after = _slots(eng)
            assert after[now][1] > max(u for _, u in before), (where, before, after)          # ... and it is the most recently used one now
        else:
            have = need = None
            if hooks and s.get("measure"):
                # what this call alone asks for (a fresh context), against the workspace the larger call before it left behind
                lone = Engine(0, test_hooks=True)
                try:
                    PH.check(s, PH.run_step(lone, s))
                    need = lone.debug_ws_bytes()
                finally:
                    lone.close()
                have = eng.debug_ws_bytes()
                RATIOS[s["call"]] = (have, need)
                print("workspace behind 256 CMZ proofs / need of %-18s %10d / %8d = %.1f" % (s["call"], have, need, have / max(need, 1)))
                assert need > 0 and have >= 8 * need, (where, have, need)
            elif hooks and (s.get("grows") or s.get("oom")):
                have = eng.debug_ws_bytes()
            if s.get("after_growth") or s.get("measure") or s.get("pair"):
                # the tables and slots of (d) are the ones prepared THEN: run_step's re-prepare (there for the lone measuring context) must find nothing to do
                assert eng.dlog_baby_bits == PH.DLOG_BABY, where
                slots = eng.dlog_point_slots()
                assert all(slots[k] == (bytes(PH.PD.base(name)), bb) for k, (name, bb) in PH.SLOTS.items()), (where, slots)
            got = PH.run_step(eng, s)
            if s.get("oom"):
                assert got is PH.Oom, where
                assert have is None or eng.debug_ws_bytes() == have, where + ": the refused call allocated"
            elif "expect" in s:
                try:
                    PH.check(s, got)
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (where, e)) from None
            if have is not None and s.get("measure"):
                assert eng.debug_ws_bytes() == have, where                   # the small call ran inside the workspace of the large one
            if have is not None and s.get("grows"):
                assert eng.debug_ws_bytes() > have, (where, have)            # ensure_ws reallocated under the live tables, slots and graph
        _nothing_runs_after_a_gpu_error(eng, where)
    assert state["graph"] is not None
    if not hooks:
        assert state["first_base_built"] == 2                                # once as the first of nine, once again behind the other eight
    else:
        assert set(RATIOS) == set(PH.CALLS)


@pytest.mark.parametrize("hooks", (False, True), ids=("shipped", "test_hooks"))
def test_one_context_through_the_whole_script(hooks):
    from zkp_amd.engine import Engine
    _torch()                                                               # (the graph steps keep their buffers in torch tensors: decided before any call)
    eng = Engine(0, test_hooks=hooks)
    try:
        _replay(eng, hooks)
    finally:
        eng.close()

"""One long-lived context through the script of tests/context_history_cases.py, on the shipped library and on the test-hook build: after
EVERY step the call's bytes are what the catalogue says (C oracle, planted verdicts, host backend -- never the device), whatever the
context went through before: larger calls, a flushed plan cache, evicted ragged bases and fixed-base tables, flipped options, a refused
call.  The GPU-only steps: a captured prove + batch-verify chain replayed with equal bytes just before the plan cache is flushed and
refused as stale ("statement plans were flushed") after it; the plan-cache size the next ragged call reports (test-hook build); the ragged
base plan that is built a second time after its eviction; and, measured with zkp_debug_ws_bytes, that the small calls behind the large ones
run in a workspace at least 8 times what they ask for on a fresh context."""
import numpy as np
import pytest

from tests import context_history_cases as H

pytestmark = pytest.mark.gpu
ZKP_ERR_ARG = -2


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch cannot see the GPU in this process (its HIP runtime must initialise before libzkp_mi355x.so: run with -m gpu)")
    return torch


class _Chain:
    """prove + batch verification of 8 DLEQ proofs on device buffers (what a graph records)"""

    def __init__(self, eng, p):
        torch = _torch()
        self.eng, self.p, self.torch = eng, p, torch
        n = p["n"]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda:0")
        self.fst = H.fused_statement(p["which"])
        table = np.concatenate([p["common"], p["inst"].reshape(-1, 32)])
        self.d_ts0, self.d_sec, self.d_tbl, self.d_ent = dev(p["ts0"]), dev(p["secrets"]), dev(table), dev(p["entropy"])
        self.d_ts, self.d_ts2 = z(n, 208), z(n, 208)
        self.d_chal, self.d_resp, self.d_coms, self.d_st = z(n, 32), z(n, 1, 32), z(n, 2, 32), z(2 * n)
        self.d_pts = z(1 + 5 * n, 32)
        self.d_pts[: 1 + 3 * n] = self.d_tbl
        self.d_w = dev(np.random.default_rng(8).integers(0, 256, size=(2, n, 16), dtype=np.uint8))
        self.d_out = z(32)
        self.d_bst = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        self.outs = (self.d_chal, self.d_resp, self.d_coms, self.d_st, self.d_out, self.d_bst, self.d_ts, self.d_ts2)

    def reset(self):
        for t in self.outs[:6]:
            t.fill_(9)
        self.d_ts.copy_(self.d_ts0)
        self.d_ts2.copy_(self.d_ts0)
        self.torch.cuda.synchronize()

    def enqueue(self):
        e, p, n = self.eng, self.p, self.p["n"]
        ptr = lambda t: t.data_ptr()
        e.fused_prove_dev(self.fst, n, p["pos"], ptr(self.d_ts), ptr(self.d_sec), ptr(self.d_tbl), ptr(self.d_ent), ptr(self.d_chal), ptr(self.d_resp), ptr(self.d_coms), ptr(self.d_st))
        e.fused_batch_verify_dev(self.fst, n, p["pos"], ptr(self.d_ts2), ptr(self.d_pts), ptr(self.d_coms), ptr(self.d_resp), ptr(self.d_w), ptr(self.d_out), ptr(self.d_bst))

    def read(self):
        self.eng.synchronize()
        return [t.cpu().numpy().copy() for t in self.outs]


def _replay(eng, hooks):
    S = H.build()
    from zkp_amd import toolbox as T
    from zkp_amd.engine import Engine
    state = {"plans": None, "graph": None}
    # sizes go down after they went up, measured (test-hook context): the first such call of every flow
    measure = {}
    for j in H.small_after_large(S):
        measure.setdefault(S[j]["kind"], j)
    measure = set(measure.values()) if hooks else set()
    assert not hooks or len(measure) == 4
    rng = np.random.default_rng(77)
    probe_ts = T.append_messages(H.LABEL, b"probe", [rng.bytes((5, 60)[j % 2]) for j in range(6)])
    th = probe_ts.copy()
    probe_want = T.hash_to_group(None, th)
    for i, s in enumerate(S):
        kind = s["kind"]
        where = "step %d (%s%s)" % (i, kind, " N=%d %s" % (s["n"], s["which"]) if "which" in s else "")
        if kind == "ragged_probe":
            ts = probe_ts.copy()
            assert (eng.fused_hash_to_group_ragged(ts) == probe_want).all() and (ts == th).all(), where
            if hooks:
                plans = eng.last_schedule()["fused_plans"]
                if s.get("dropped"):
                    assert plans == 1 and plans < state["plans"], (where, plans, state["plans"])       # the flushing call's plan alone
                state["plans"] = plans
        elif kind == "graph_capture":
            p = s["p"]
            ch = _Chain(eng, p)
            ch.reset()
            ch.enqueue()
            direct = ch.read()
            assert (direct[0] == p["chal"]).all() and (direct[1] == p["resp"]).all() and (direct[2] == p["coms"]).all(), where    # the oracle's proofs
            assert not direct[3].any() and not direct[4].any() and not direct[5].any(), where                                     # ... accepted as a batch
            ch.reset()
            with eng.capture() as cap:
                ch.enqueue()
            ch.read()
            ch.reset()
            cap.graph.launch()
            replayed = ch.read()
            for a, b in zip(direct, replayed):
                assert (a == b).all(), where
            state["graph"], state["chain"] = cap.graph, ch
        elif kind == "graph_stale":
            g = state["graph"]
            rc = eng._lib.zkp_graph_launch(g._h, eng._h)
            assert rc == ZKP_ERR_ARG and "statement plans were flushed" in eng._lib.zkp_last_error().decode(), where
            g.close()
        else:
            if i in measure:
                # what this call alone asks for (a fresh context), against the workspace the larger call before it left behind
                lone = Engine(0, test_hooks=True)
                try:
                    H.check(s, H.run_step(lone, s))
                    need = lone.debug_ws_bytes()
                finally:
                    lone.close()
                have = eng.debug_ws_bytes()
                assert need > 0 and have >= 8 * need, (where, have, need)
            got = H.run_step(eng, s)
            if i in measure:
                assert eng.debug_ws_bytes() == have, where                 # the small call ran inside the workspace of the large one
            if s.get("oom"):
                assert got is H.Oom, where
            elif "expect" in s:
                try:
                    H.check(s, got)
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (where, e)) from None
            if hooks and s.get("base"):
                sched = eng.last_schedule()
                assert sched.get("ragged_base") == (1 if s.get("rebuilds_base") or not any(t.get("base") == s["base"] for t in S[:i]) else 0), (where, sched)
    assert state["graph"] is not None


@pytest.mark.parametrize("hooks", (False, True), ids=("shipped", "test_hooks"))
def test_one_context_through_the_whole_script(hooks):
    from zkp_amd.engine import Engine
    _torch()                                                               # (the graph steps keep their buffers in torch tensors: decided before any call)
    eng = Engine(0, test_hooks=hooks)
    try:
        _replay(eng, hooks)
    finally:
        eng.close()

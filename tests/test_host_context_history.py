"""The script of tests/context_history_cases.py without a GPU: every step on the toolbox's host backend gives what the catalogue expects
(so catalogue = host backend = C oracle = planted verdicts), and the script really drives a context through the transitions it is
there for -- each coverage condition is an assertion on the script's own data."""
import numpy as np

from tests import context_history_cases as H

GPU_ONLY = ("ragged_probe", "graph_capture", "graph_stale")
CALLS = ("prove", "verify_compact", "verify_each", "batch")


def _script():
    return H.build()


def test_every_step_on_the_host_backend_gives_the_catalogued_result():
    n_checked = 0
    for s in _script():
        if s["kind"] in GPU_ONLY or s.get("oom") or s.get("mode") == "discard":       # (no host route: a refused call, a job nobody waits for)
            continue
        got = H.run_step(None, s)
        if "expect" in s:
            H.check(s, got)
            n_checked += 1
    assert n_checked >= 120


def test_expectations_come_from_the_oracle_the_planted_set_or_the_host_backend():
    for s in _script():
        if "expect" in s:
            assert s["source"] in ("oracle", "planted", "host")
            assert s["source"] != "host" or (s["kind"] == "prove" and s["ragged"])       # only ragged proofs lean on the host backend


def test_sizes_go_down_after_they_went_up():
    """every flow is called at N <= 65 right after a call of a DIFFERENT flow that touches at least 8 times as many operands"""
    S = _script()
    # (operands per call stand in for the workspace need here; tests/test_gpu_context_history.py measures the need itself at these steps)
    assert {S[i]["kind"] for i in H.small_after_large(S)} == set(CALLS)


def test_plan_cache_is_flushed_once_with_a_graph_captured_just_before():
    S = _script()
    keys, flush_at = [], None
    for i, s in enumerate(S):
        k = s.get("key")
        if k and k not in keys:
            if len(keys) == H.PLAN_CAP:
                assert flush_at is None and s.get("flushes"), "the 65th distinct plan must be the step marked as flushing"
                flush_at = i
                before = list(keys)
            keys.append(k)
        else:
            assert not s.get("flushes") or k in keys[-1:]
    assert len(keys) >= 70 and flush_at is not None
    assert sum(1 for s in S if s.get("flushes")) == 1
    assert S[flush_at - 1]["kind"] == "graph_capture"
    cap = S[flush_at - 1]["p"]
    assert ("P", cap["which"], cap["n"], cap["pos"]) in before and ("B", cap["which"], cap["n"], cap["pos"]) in before      # the chain's plans exist: the capture compiles nothing
    assert [s["kind"] for s in S[flush_at + 1:flush_at + 3]] == ["graph_stale", "ragged_probe"] and S[flush_at + 2]["dropped"]
    assert any(s["kind"] == "ragged_probe" and not s.get("dropped") for s in S[:flush_at])
    again = S[flush_at + 3]
    assert again.get("repeat_of") == 0 and again["key"] == S[0]["key"] == before[0] and again["expect"] is S[0]["expect"]
    # the flushing call is smaller than calls that came before the capture: it cannot grow the workspace (a graph that is stale for THAT reason says so first)
    units = lambda s: s["n"] * H.TERMS[(s["kind"], s["which"])]
    assert 8 * units(S[flush_at]) <= max(units(s) for s in S[:flush_at - 1] if s["kind"] in CALLS)


def test_ragged_base_cache_evicts_the_first_base_before_it_is_called_again():
    S = _script()
    cache, tick = {}, 0
    rebuilt = []
    for s in S:
        b = s.get("base")
        if not b:
            continue
        tick += 1
        if b not in cache:
            rebuilt.append(b)
        cache[b] = tick
        while len(cache) > H.RAGGED_BASE_CAP:
            del cache[min((v, k) for k, v in cache.items() if v != tick)[1]]
        assert bool(s.get("rebuilds_base")) == (rebuilt.count(b) == 2 and rebuilt[-1] == b)
    assert len(set(rebuilt)) >= 66
    last = [s for s in S if s.get("rebuilds_base")]
    assert len(last) == 1 and last[0]["base"] == rebuilt[0]


def test_fixed_base_slots_are_registered_evicted_and_registered_again():
    S = _script()
    regs = [i for i, s in enumerate(S) if s["kind"] == "register"]
    valid = lambda e: bytes(e) != bytes(H.JUNK)
    distinct = {bytes(e) for i in regs for e in S[i]["encodings"] if valid(e)}
    assert len(distinct) >= 130
    assert any(any(bytes(e) == bytes(H.JUNK) for e in S[i]["encodings"]) and any(not e.any() for e in S[i]["encodings"]) for i in regs)
    # the library's replacement rule (free slots first, then least recently used, never a slot this call touched) on the host
    slots, used, tick, state = [None] * H.HOT_SLOTS, [0] * H.HOT_SLOTS, 0, []
    common = {bytes(e) for e in S[regs[0]]["encodings"]}
    for i in regs:
        tick += 1
        fresh = []
        for e in map(bytes, S[i]["encodings"]):
            if e in slots:
                used[slots.index(e)] = tick
            elif e not in fresh:
                fresh.append(e)
        for e in fresh[:H.HOT_SLOTS]:
            if e == bytes(H.JUNK):
                continue
            free = [k for k in range(H.HOT_SLOTS) if used[k] != tick]
            if not free:
                break
            k = next((k for k in free if slots[k] is None), min(free, key=lambda k: used[k]))
            slots[k], used[k] = e, tick
        state.append(sum(e in slots for e in common))
        follow = S[i + 1:i + 4]
        assert [s["kind"] for s in follow] == ["msm_many", "msm_many", "prove"] and [follow[0]["flags"], follow[1]["flags"]] == [1, 0]
        assert follow[2]["which"] == "cmz" and {bytes(e) for e in follow[2]["p"]["common"]} == common
        assert {bytes(e) for e in follow[0]["points"]} == common
    assert state[0] == len(common) and state[1] == 0 and state[2] == 0 and state[3] == len(common), state


def test_options_are_flipped_between_equal_calls():
    S = _script()
    want = {"JOINT_LADDER": [0, 2, 1], "TRANSCRIPT_STEPS": [0, 1], "TRANSCRIPT_LANES": [1, 2], "FUSE_TABLES_TRANSCRIPT": [0, 1, 2, 0], "COMB_SPLIT": [0, 1, 2, 0],
            "EACH_STRAUS": [0, 1, 2, 0], "CT_LOOKUP": [0, 1, 2, 0], "SYNC_SCHEDULE": [1, 0]}
    for name, values in want.items():
        at = [i for i, s in enumerate(S) if s["kind"] == "option" and s["name"] == name]
        assert [S[i]["value"] for i in at][:len(values)] == values, name
        for i in at:
            a, b = S[i - 1], S[i + 1]
            assert a["kind"] == b["kind"] and a["kind"] in CALLS and a["key"] == b["key"] and a["expect"] is not None
            assert all(np.array_equal(x, y) for x, y in zip(np.atleast_1d(a["expect"]), np.atleast_1d(b["expect"]))) if not isinstance(a["expect"], tuple) else \
                all(np.array_equal(x, y) for x, y in zip(a["expect"], b["expect"]))
        # the plan of the probed call exists before the first flip
        assert any(s.get("key") == S[at[0] - 1]["key"] for s in S[:at[0]])


def test_verdicts_alternate_with_another_flow_in_between():
    S = _script()
    for kind in ("verify_compact", "verify_each", "batch"):
        sizes = set()
        for i in range(len(S) - 6):
            run = S[i:i + 7:2]
            if all(s["kind"] == kind and not s["ragged"] for s in run) and len({s["n"] for s in run}) == 1:
                rejected = [bool(np.asarray(s["expect"]).any()) for s in run]
                between = S[i + 1:i + 7:2]
                if rejected == [True, False, True, False] and all(b["kind"] in CALLS and b["kind"] != kind for b in between):
                    sizes.add(run[0]["n"])
        assert len(sizes) >= 2, (kind, sizes)


def test_a_job_is_waited_for_and_a_job_is_discarded_between_synchronous_calls():
    S = _script()
    jobs = [i for i, s in enumerate(S) if s["kind"] == "job"]
    assert [S[i]["mode"] for i in jobs] == ["wait", "discard"]
    w, d = jobs
    for i in jobs:
        assert S[i - 1]["kind"] in CALLS and S[i + 1]["kind"] in CALLS and "expect" in S[i + 1]
    assert 0 < int(S[w]["expect"].sum()) < S[w]["n"]                              # the waited job rejects some proofs and accepts the others
    # the discarded job would have accepted proofs: its verdict words must still say "rejected" for every one of them
    assert S[d]["expect"].all() and not S[d]["verdicts_if_waited"].all()
    after = S[d + 1]
    assert (after["kind"], after["key"]) == ("verify_compact", S[d]["key"]) and not after["expect"].all() and after["expect"].any()
    assert not np.array_equal(after["expect"], S[d]["verdicts_if_waited"])        # nor can it pass on what the discarded job left on the device


def test_workspace_limit_refuses_then_lets_the_smaller_and_the_lifted_call_through():
    S = _script()
    i = next(i for i, s in enumerate(S) if s["kind"] == "option" and s["name"] == "WS_LIMIT_BYTES" and s["value"])
    big, small, lift, again = S[i + 1], S[i + 2], S[i + 3], S[i + 4]
    assert big.get("oom") and big["kind"] in CALLS and small["kind"] in CALLS and "expect" in small and not small.get("oom")
    assert lift["kind"] == "option" and lift["name"] == "WS_LIMIT_BYTES" and lift["value"] == 0
    assert again["key"] == big["key"] and not again.get("oom")
    largest = max(s["n"] * H.TERMS[(s["kind"], s["which"])] for s in S[:i] if s["kind"] in CALLS)
    assert big["n"] * H.TERMS[(big["kind"], big["which"])] >= 2 * largest          # the refused call would have had to grow the workspace
    assert small["n"] * H.TERMS[(small["kind"], small["which"])] < largest

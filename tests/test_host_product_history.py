"""The script of tests/product_history_cases.py without a GPU: every step on the toolbox with ctx == NULL gives what the catalogue expects, so
the catalogue (C oracle, oracle.model in Python, Python integers, chosen logarithms, planted verdicts) and the host route of every product call
agree, and the script really drives a context through the transitions it is there for -- each is an assertion on the script's own data."""
import numpy as np
import pytest

from tests import product_history_cases as PH

GPU_ONLY = ("graph_capture", "graph_replay", "graph_stale")
PROOF_CALLS = ("prove", "verify_compact", "verify_each", "batch")
SOURCES = ("oracle", "python", "model", "cases", "chosen", "planted", "refused")


def _script():
    return PH.build()


def test_every_step_on_the_host_route_gives_the_catalogued_result():
    n_checked = 0
    for s in _script():
        if s["kind"] in GPU_ONLY or s.get("oom"):                               # (no host route: the graph steps, the call the limit refuses)
            continue
        got = PH.run_step(None, s)
        if "expect" in s:
            PH.check(s, got)
            n_checked += 1
    assert n_checked >= 300


def test_every_expectation_has_a_source_that_is_neither_the_host_backend_nor_the_device():
    for s in _script():
        if "expect" in s or s["kind"] in GPU_ONLY[:2]:
            assert s["source"] in SOURCES, s.get("name", s["kind"])
    assert {s["call"] for s in _script() if s["kind"] == "product"} == set(PH.CALLS)


def test_a_corrupted_expectation_is_reported_with_the_name_of_its_step():
    s = dict(PH.product_step("sc_muladd", PH.N_BIG))
    bad = s["expect"].copy()
    bad[17, 3] ^= 1
    s["expect"] = bad
    with pytest.raises(AssertionError, match=r"sc_muladd n=65 \(source: python\): result 0 differs in rows \[17\]"):
        PH.check(s, PH.run_step(None, s))
    s = dict(PH.product_step("tr_chal_scalars", PH.N_SMALL))
    out, ts = s["expect"]
    ts = ts.copy()
    ts[4, 100] ^= 0x80
    s["expect"] = (out, ts)
    with pytest.raises(AssertionError, match=r"tr_chal_scalars n=9 .*result 1 differs in rows \[4\]"):
        PH.check(s, PH.run_step(None, s))


def test_transcripts_stand_at_a_mix_of_positions_with_the_last_of_a_block_among_them():
    for c in PH.FAMILIES["transcript"]:
        pos = PH.product_step(c, PH.N_BIG)["ts"][:, 200]
        assert pos[0] == 165 and len(set(pos.tolist())) >= 40, c


def test_a_the_products_follow_the_large_proof_flow_each_one_measured_once():
    S = _script()
    at = [i for i, s in enumerate(S) if s.get("measure")]
    assert [S[i]["call"] for i in at] == list(PH.CALLS) and at == list(range(at[0], at[0] + len(PH.CALLS)))
    big = S[at[0] - 1]
    assert (big["kind"], big["which"], big["n"]) == ("prove", "cmz", 256)
    assert all(S[i]["n"] == PH.N_BIG for i in at)


def test_b_the_proof_flows_follow_the_block_of_products():
    S = _script()
    i = next(i for i, s in enumerate(S) if s.get("after_products"))
    assert S[i - 1].get("measure") and (S[i]["kind"], S[i]["which"], S[i]["n"]) == ("prove", "cmz", 64)
    kinds = [s["kind"] for s in S[i + 1:i + 4]]
    assert kinds == ["verify_compact", "verify_each", "batch"]
    for s in S[i + 1:i + 4]:
        assert s["mutants"] and s["source"] == "planted" and 0 < int(np.asarray(s["expect"]).sum()) < len(s["expect"])


def test_c_every_product_call_is_followed_by_each_other_family_at_a_smaller_size():
    S = _script()
    seen = set()
    for i, s in enumerate(S[:-1]):
        if s.get("pair"):
            nxt = S[i + 1]
            assert nxt["kind"] == "product" and nxt["family"] == s["pair"][1] != s["family"] and nxt["n"] < s["n"]
            seen.add(s["pair"])
    assert seen == {(c, f) for c in PH.CALLS for f in PH.FAMILIES if f != PH.FAMILY_OF[c]}


def test_d_growth_comes_after_the_tables_slots_and_the_recorded_graph_and_before_their_next_use():
    S = _script()
    k = [s["kind"] for s in S]
    reg, first, prep, cap, rep, stale = k.index("register"), next(i for i, s in enumerate(S) if s.get("first_mul_base")), k.index("prepare_dlog"), \
        k.index("graph_capture"), k.index("graph_replay"), k.index("graph_stale")
    slots = [i for i, s in enumerate(S) if s["kind"] == "prepare_dlog_point"]
    grow = next(i for i, s in enumerate(S) if s.get("grows"))
    assert reg < first < prep < slots[0] < slots[1] < cap < rep < grow < stale
    assert not any(s.get("call") == "mul_base" for s in S[:first])
    assert [(S[i]["slot"], S[i]["baby_bits"]) for i in slots] == [(0, 4), (7, 8)]
    assert [bytes(S[i]["base"]) for i in slots] == [PH.PD.base("G7"), PH.PD.base("H")]
    assert [s["call"] for s in S[cap - 5:cap]] == list(PH.GRAPH_CALLS) and all(s["n"] == PH.N_BIG for s in S[cap - 5:cap])
    between = S[cap + 1:rep]
    assert len(between) >= 5 and all(s["kind"] == "product" and s["n"] < PH.N_BIG and s["call"] in PH.GRAPH_CALLS for s in between)
    # nothing before the growing call is a proof flow or a call of more than a few megabytes: 256 CMZ proofs outgrow all of it
    assert not any(s["kind"] in PROOF_CALLS for s in S[:grow]) and (S[grow]["which"], S[grow]["n"]) == ("cmz", 256)
    after = S[grow + 1:stale]
    assert all(s.get("after_growth") for s in after)
    assert [s.get("call", s["kind"]) for s in after] == ["dlog_base", "dlog_point", "dlog_point", "dlog_point", "dlog_point", "mul_base", "msm_many", "prove"]
    assert [(s["slot"], s["signed"]) for s in after[1:5]] == [(0, False), (0, True), (7, False), (7, True)]
    assert after[6]["flags"] == 1 and {bytes(e) for e in after[6]["points"]} == {bytes(e) for e in S[reg]["encodings"]}


def test_e_nine_bases_go_through_the_toolbox_with_a_verification_between_and_the_first_comes_again():
    S = _script()
    at = [i for i, s in enumerate(S) if s["kind"] == "dlog_toolbox"]
    bases = [bytes(S[i]["base"]) for i in at]
    assert len(at) == 10 and len(set(bases[:9])) == 9 and bases[9] == bases[0] and S[at[9]]["again"]
    assert {PH.PD.base(n) for n in PH.PD.BASES} <= set(bases)
    for i in at:
        assert S[i + 1]["kind"] == "verify_compact" and S[i + 1]["which"] == "dleq"
    assert at[0] > max(i for i, s in enumerate(S) if s["kind"] == "prepare_dlog_point")


def test_f_a_refused_call_stands_between_two_good_ones_per_family_and_the_limit_refuses_a_product_call():
    S = _script()
    at = [i for i, s in enumerate(S) if s["kind"] == "refused"]
    assert [S[i]["family"] for i in at] == ["scalar", "transcript", "pairwise", "fold", "scan", "dlog"]
    for i in at:
        assert S[i - 1]["kind"] == S[i + 1]["kind"] == "product" and S[i - 1]["family"] == S[i + 1]["family"] == S[i]["family"]
    i = next(i for i, s in enumerate(S) if s["kind"] == "option" and s["name"] == "WS_LIMIT_BYTES" and s["value"])
    assert S[i]["value"] == 1 << 20 and S[i + 1].get("oom") and S[i + 1]["kind"] == "product"
    assert 32 * int(S[i + 1]["off"][-1]) > 1 << 20                               # its input alone is more than the limit
    assert S[i + 2]["kind"] == "product" and not S[i + 2].get("oom")
    assert (S[i + 3]["kind"], S[i + 3]["name"], S[i + 3]["value"]) == ("option", "WS_LIMIT_BYTES", 0)
    assert S[i + 4]["expect"] is S[i + 1]["expect"] and not S[i + 4].get("oom")
    assert not any(s["kind"] in PROOF_CALLS for s in S[:i])                      # nothing large came first: the refused call would have had to grow


def test_g_options_are_flipped_between_equal_product_calls_and_flipped_back():
    S = _script()
    want = {"BATCH_ENCODE_MIN": [0, 65536], "COMB_TEETH": [16, 8, 4], "GROUPED_COMB": [1, 0, PH.DEFAULT], "TABLES_LANE": [1, 0, PH.DEFAULT],
            "CT_SINGLE_USE_TABLES": [1, 0, PH.DEFAULT], "LADDER_INTERLEAVE": [1, 0, PH.DEFAULT], "COMB_SPLIT": [1, 0, PH.DEFAULT]}
    for name, values in want.items():
        at = [i for i, s in enumerate(S) if s["kind"] == "option" and s["name"] == name]
        assert [S[i]["value"] for i in at] == values, name
        for i in at:
            a, b = S[i - 1], S[i + 1]
            assert a["kind"] == b["kind"] == "product" and a["call"] == b["call"] == "msm_segments" and a["expect"] is b["expect"]
            assert a["flags"] == 1 and int(a["off"][-1]) >= 1024                 # constant time, on the classified term path
    assert [s["value"] for s in S if s["kind"] == "option" and s.get("refused")] == [8]

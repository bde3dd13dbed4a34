"""Random statement shapes (tests/random_statements.py: twelve families built for one class edge each, twelve seeded random statements) on
every term path and schedule.  pair_terms, cfg_from_terms / pick_teeth and k_stmt_classify decide from the statement's shape alone how each
term of a batch is computed, and the host bounds and the device classification must agree exactly; the rest of the suite drives them with
CMZ and a few hand-written shapes.  Here every statement runs at 6 proofs (both jobs below 1,024 terms: the generic classifier) and at 66 or
more (both at or above: the one-launch classifier, more than a wavefront of proofs) through
  (a) the synchronous toolbox route (host transcripts with device MSMs, and fused) under the options that change a term path or a schedule,
  (b) the _dev entry points under every configuration of tests/test_gpu_degenerate.py, common points registered and not (families),
  (c) the test-hook build with the one-launch classifier and with the generic path's atomics classifier (an independent implementation of the
      same decision), where zkp_debug_last_schedule confirms the path each family was built for.
Everything is compared with oracle/c: proofs byte for byte, verdicts proof by proof with one tampered response per batch (on a term that
rides where the statement has one), the batch verifier's operand scalars, the transcripts left behind.  The oracle's expectations are
computed once per (statement, n) and shared (random_statements.expectation); tests/test_host_random_statements.py proves them without a GPU."""
import pytest

from zkp_amd import engine as EN
from zkp_amd import toolbox as T
from tests import random_statements as R
from tests import statement_shapes as SH
from tests.test_gpu_degenerate import DEV_CONFIGS

pytestmark = pytest.mark.gpu
O = EN
SYNC_CONFIGS = {
    "default": {},
    "separate_terms": {O.ZKP_OPT_JOINT_LADDER: 0},
    "pairs_without_tables": {O.ZKP_OPT_JOINT_LADDER: 2},
    "pairs+riders_tables": {O.ZKP_OPT_JOINT_LADDER: 1, O.ZKP_OPT_SYNC_SCHEDULE: 1},
    "grouped+single_use_ladder": {O.ZKP_OPT_GROUPED_COMB: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0},
    "grouped+single_use_tables": {O.ZKP_OPT_GROUPED_COMB: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 1},
    "comb_split": {O.ZKP_OPT_COMB_SPLIT: 1},
    "masked_scans+grouped": {O.ZKP_OPT_CT_LOOKUP: 1, O.ZKP_OPT_GROUPED_COMB: 1},
    "interp": {O.ZKP_OPT_TRANSCRIPT_STEPS: 0},
    "one_lane": {O.ZKP_OPT_TRANSCRIPT_LANES: 1},
    "each_straus_off": {O.ZKP_OPT_EACH_STRAUS: 0},
    "each_straus_3_lanes": {O.ZKP_OPT_EACH_STRAUS: 3},
    "each_straus_4_window_parts": {O.ZKP_OPT_EACH_STRAUS: 0x204},
    "batch_encode_all": {O.ZKP_OPT_BATCH_ENCODE_MIN: 0},
}
PARTS = {"families": list(R.FAMILIES), "random": list(R.SEEDS)}


def _configure(e, opts):
    """ZKP_OPT_CT_LOOKUP 1 (masked scans) exists in builds with 6-bit fixed-base windows only; the shipped library has 7-bit windows and refuses
    the value without changing anything (tests/context_history_cases.py).  The statements then run under the rest of the configuration."""
    for opt, v in opts.items():
        if opt == O.ZKP_OPT_CT_LOOKUP and v:
            try:
                e.set_option(opt, v)
            except EN.ZkpError as err:
                assert "6-bit" in str(err), err
            continue
        e.set_option(opt, v)


# ---- (a) the synchronous toolbox route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("config", list(SYNC_CONFIGS))
def test_toolbox_routes_on_every_term_path_and_schedule(config, part):
    e = EN.Engine(0)                                                       # a fresh context per configuration: no option has to be restored
    try:
        _configure(e, SYNC_CONFIGS[config])
        for key in PARTS[part]:
            for n in R.sizes(key):
                R.check_statement(e, key, n)
    finally:
        e.close()
        T.set_fused_min_batch(32)


# ---- (b) the _dev entry points ----------------------------------------------------------------------------------------------------------------------
def _dev_statement(e, key, n, register, after=None):
    b, E, E_bad = R.expectation(key, n)
    assert R.honest(E), "the oracle refuses its own honest proofs of %r at n = %d" % (key, n)
    try:
        SH.dev_flows(e, None, b, E, register=register, after=after)
        SH.dev_flows(e, None, b, E_bad, names={E_bad.bad: "one response tampered"}, register=register, prove=False)
    except AssertionError as err:
        raise AssertionError("statement %r, n = %d: %s" % (key, n, err)) from err


@pytest.mark.parametrize("register", [True, False], ids=["registered", "unregistered"])
@pytest.mark.parametrize("config", list(DEV_CONFIGS))
def test_dev_entry_points_on_every_schedule_and_term_path(config, register):
    e = EN.Engine(0)
    try:
        _configure(e, DEV_CONFIGS[config])
        for key in R.FAMILIES:
            for n in R.sizes(key):
                _dev_statement(e, key, n, register)
    finally:
        e.close()


# ---- (c) the one-launch classifier against the generic path's ----------------------------------------------------------------------------------------
HOOK_CONFIGS = {
    "pairs+riders_tables": ({O.ZKP_OPT_JOINT_LADDER: 1, O.ZKP_OPT_SYNC_SCHEDULE: 1}, 1, None),
    "grouped+single_use_ladder": ({O.ZKP_OPT_GROUPED_COMB: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 0}, 2, 1),
    "grouped+single_use_tables": ({O.ZKP_OPT_GROUPED_COMB: 1, O.ZKP_OPT_CT_SINGLE_USE_TABLES: 1}, 1, 1),
}                                                                            # options, the comb_min the prover asks for, grouped


@pytest.mark.parametrize("config", list(HOOK_CONFIGS))
def test_both_classifiers_give_the_oracles_bytes_on_the_path_each_family_was_built_for(config):
    """Both runs are compared with the oracle byte for byte, hence with each other.  The schedule words are read after the prover and after
    verify_compact: the _dev calls run the throughput schedule, which builds the riders' tables wherever the census says the job has 16 teeth."""
    opts, ask, grouped = HOOK_CONFIGS[config]
    seen = {}
    for generic in (0, 1):
        e = EN.Engine(0, test_hooks=True)
        try:
            _configure(e, opts)
            e.set_option(EN.ZKP_TESTOPT_GENERIC_CLASSIFIER, generic)
            for key in R.FAMILIES:
                for n in R.sizes(key):
                    p, v = R.census(R.statement(key), "prove"), R.census(R.statement(key), "verify")
                    if n * p.T < R.STMT_MIN_TERMS:
                        continue
                    sched = {}
                    _dev_statement(e, key, n, False, after=lambda what: sched.setdefault(what, e.last_schedule()))
                    sp, sv = sched["prove"], sched["verify_compact"]
                    where = (key, n, generic, sp, sv)
                    assert sp.get("terms_split") == 1 and sv.get("terms_split") == 1, where
                    assert sp.get("comb_min") == p.comb_min(ask) and sv.get("comb_min") == 2, where
                    if grouped is not None:
                        assert sp.get("grouped") == grouped, where
                    if generic or v.pair is None:
                        assert "riders" not in sv, where                 # no pairs outside the one-launch classifier, or nothing to pair
                    else:
                        assert sv.get("riders") == int(v.rider_ok(n, riders=True)), where
                    assert "riders" not in sp, where
                    # a call says whether its ladder blocks interleave only when its bounds hold a ladder: the plan's ladder bound is zero exactly
                    # where the census has no single-use point (the generic run pairs nothing, so the verifier's census is the unpaired one)
                    vb = (R.census(R.statement(key), "verify", pairs=False) if generic else v).bounds(n, 2, riders=not generic)
                    assert ("ladder_interleave" in sp) == (p.bounds(n, ask)["n_lad"] > 0), where
                    assert ("ladder_interleave" in sv) == (vb["n_lad"] > 0), where
                    seen[(key, n, generic)] = (sp, sv)
                    print("%s n=%d generic=%d prove: %s | verify_compact: %s" % (key, n, generic, " ".join("%s=%d" % kv for kv in sp.items()),
                                                                                  " ".join("%s=%d" % kv for kv in sv.items())))
        finally:
            e.close()
    big = lambda key: R.sizes(key)[1]
    assert seen[("rider_at_min", big("rider_at_min"), 0)][1]["riders"] == 1
    assert seen[("four_teeth_with_pairs", big("four_teeth_with_pairs"), 0)][1]["riders"] == 0
    assert sum(1 for (key, n, g), (sp, sv) in seen.items() if g == 0 and "riders" in sv) >= 10

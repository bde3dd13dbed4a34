"""(helper module of tests/test_host_size_thresholds.py and tests/test_gpu_thresholds.py)
Every size threshold by which the library picks a kernel, a workspace layout or a status protocol for a call, with the sizes on both
sides of it that the GPU test runs.  The library promises that these choices never change a result (include/zkp_mi355x.h); the GPU
test checks that the default choice really flips at the boundary (zkp_debug_last_schedule of the test-hook build), that the default
bytes equal the bytes of every forced choice and of the shipped library, and checks the results against the oracle.  The CPU test
parses the thresholds out of the sources and fails when one of them has no row here with the same value.

Fields of a row:
  row       the row number of the threshold table (test ids start with it)
  name      short name of the decision (test ids: "<row>-<name>-<size>-<schedule>")
  const     the constant or literal the sources compare against (a name, or the literal as written, e.g. "1u << 18")
  value     its value
  source    file under zkp_amd/csrc that makes the decision
  entry     how the GPU test reaches it: msm_many (host pointers), msm_many_dev (device pointers, the throughput schedule),
            msm_optional, batch_verify (K = 1, DLEQ), and the fused _dev flows: prove (DLEQ), prove_cmz (CMZ, the flows' own
            workspace sizing of rows 6 - 8), verify_compact (CMZ), verify_batchable (DLEQ), verify_batchable_w64 (w64_statement:
            Q = sum of 64 x_i G_i, 66 operands per proof)
  schedule  "latency" (synchronous host-pointer entry points; the _dev flows with ZKP_OPT_DEV_OVERLAP = 2) or "throughput"
  sizes     the call sizes to run: terms, outputs or proofs as the row says (unit)
  unit      what a size counts
  key       the key of zkp_debug_last_schedule that reports the choice
  expect    the value the key must have at each size (same order as sizes)
  option    (ZKP_OPT_* number, [values]) that forces each explicit choice, or None
  unreachable  None, or why no default call can reach the boundary (the GPU test skips such rows)
"""

ROWS = [
    # ---- term path (zkp_kernels.hip: msm_terms_path) ----------------------------------------------------------------------------------
    dict(row=0, name="terms_split", const="n_terms >= 1024", value=1024, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(1023, 1024), unit="terms", key="terms_split", expect=(0, 1), option=None, unreachable=None),
    dict(row=1, name="batch_encode", const="batch_encode_min", value=65536, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(65535, 65536), unit="outputs", key="batch_encode", expect=(0, 1), option=(1, (0, 2**64 - 1)), unreachable=None),
    dict(row="1b", name="batch_encode", const="kThroughputEncodeMin", value=2048, source="zkp_kernels.hip", entry="msm_many_dev", schedule="throughput",
         sizes=(2047, 2048), unit="outputs", key="batch_encode", expect=(0, 1), option=None, unreachable=None),
    dict(row=2, name="enc_groups", const="ENC_BLOCK", value=256, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(65536, 65537, 131072, 131073), unit="outputs", key="enc_groups", expect=(1, 2, 2, 3), option=None, unreachable=None),
    dict(row=3, name="opt_pip", const="kSmallOptional", value=192, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=(192, 193), unit="terms", key="opt_pip", expect=(0, 1), option=None, unreachable=None),
    # batch verification, K = 1: status words without memsets once the MSM has more than kSmallOptional terms.  A DLEQ batch MSM has
    # 1 + 5 N terms: N = 38 (191 terms) and 39 (196) are the nearest sizes on each side
    dict(row="3b", name="status_shared", const="kSmallOptional", value=192, source="fused_flows.h", entry="batch_verify", schedule="throughput",
         sizes=(38, 39), unit="proofs", key="status_shared", expect=(0, 1), option=None, unreachable=None),
    dict(row=4, name="pip_c", const="1u << 12", value=1 << 12, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=(4095, 4096), unit="terms", key="pip_c", expect=(7, 10), option=None, unreachable=None),
    dict(row=4, name="pip_c", const="1u << 13", value=1 << 13, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=(8191, 8192), unit="terms", key="pip_c", expect=(10, 11), option=None, unreachable=None),
    dict(row=4, name="pip_c", const="1u << 21", value=1 << 21, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=((1 << 21) - 1, 1 << 21), unit="terms", key="pip_c", expect=(11, 16), option=None, unreachable=None),
    dict(row=5, name="pip_part", const="1u << 18", value=1 << 18, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=((1 << 18) - 1, 1 << 18), unit="terms", key="pip_part", expect=(16, 32), option=None, unreachable=None),
    dict(row=5, name="pip_part", const="1u << 21", value=1 << 21, source="zkp_kernels.hip", entry="msm_optional", schedule="latency",
         sizes=((1 << 21) - 1, 1 << 21), unit="terms", key="pip_part", expect=(32, 64), option=None, unreachable=None),
    # constant-time calls: quad-split comb scans + grouped walk on the latency schedule between kSplitCombTerms and kGroupedCombTerms terms
    dict(row=6, name="lat_split", const="kSplitCombTerms", value=8192, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(8191, 8192), unit="terms", key="lat_split", expect=(0, 1), option=(16, (0, 1)), unreachable=None),
    dict(row=6, name="lat_split", const="kGroupedCombTerms", value=400000, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(399999, 400000), unit="terms", key="lat_split", expect=(1, 0), option=(16, (0, 1)), unreachable=None),
    # grouped comb walk: from kSplitCombTerms (with lat_split) on the latency schedule -- at kGroupedCombTerms the split ends and the size
    # rule takes over, so the walk stays on across that boundary -- and from kWideCallTerms on the throughput schedule
    dict(row=7, name="grouped", const="kSplitCombTerms", value=8192, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(8191, 8192), unit="terms", key="grouped", expect=(0, 1), option=(6, (0, 1)), unreachable=None),
    dict(row=7, name="grouped", const="kGroupedCombTerms", value=400000, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(399999, 400000), unit="terms", key="grouped", expect=(1, 1), option=(6, (0, 1)), unreachable=None),
    dict(row=7, name="grouped", const="kWideCallTerms", value=250000, source="zkp_kernels.hip", entry="msm_many_dev", schedule="throughput",
         sizes=(249999, 250000), unit="terms", key="grouped", expect=(0, 1), option=(6, (0, 1)), unreachable=None),
    # single-use points of constant-time calls: comb tables (comb_min 1) below kWideCallTerms terms on the throughput schedule, the ladder (2) from there
    dict(row=8, name="comb_min", const="kWideCallTerms", value=250000, source="zkp_kernels.hip", entry="msm_many_dev", schedule="throughput",
         sizes=(249999, 250000), unit="terms", key="comb_min", expect=(1, 2), option=(3, (0, 1)), unreachable=None),
    # ladder blocks spread over the grid from kInterleaveLadderBlocks blocks of 256 single-use points (variable time: they always take the ladder)
    # the same rules in the CMZ prove flow (31 terms per proof: N = 264 / 265, 8064 / 8065, 12903 / 12904 are the nearest N on each side),
    # whose workspace is sized by prove_terms_cfg, not by the msm_many path's host_terms_cfg
    dict(row=6, name="lat_split", const="kSplitCombTerms", value=8192, source="zkp_kernels.hip", entry="prove_cmz", schedule="latency",
         sizes=(264, 265), unit="proofs", key="lat_split", expect=(0, 1), option=(16, (0, 1)), unreachable=None),
    dict(row=6, name="lat_split", const="kGroupedCombTerms", value=400000, source="zkp_kernels.hip", entry="prove_cmz", schedule="latency",
         sizes=(12903, 12904), unit="proofs", key="lat_split", expect=(1, 0), option=(16, (0, 1)), unreachable=None),
    dict(row=7, name="grouped", const="kWideCallTerms", value=250000, source="zkp_kernels.hip", entry="prove_cmz", schedule="throughput",
         sizes=(8064, 8065), unit="proofs", key="grouped", expect=(0, 1), option=(6, (0, 1)), unreachable=None),
    dict(row=8, name="comb_min", const="kWideCallTerms", value=250000, source="zkp_kernels.hip", entry="prove_cmz", schedule="throughput",
         sizes=(8064, 8065), unit="proofs", key="comb_min", expect=(1, 2), option=(3, (0, 1)), unreachable=None),
    dict(row=9, name="ladder_interleave", const="kInterleaveLadderBlocks", value=256, source="zkp_kernels.hip", entry="msm_many", schedule="latency",
         sizes=(65280, 65281), unit="single-use points", key="ladder_interleave", expect=(0, 1), option=(11, (0, 1)), unreachable=None),
    # ---- fused flows (fused_flows.h) ------------------------------------------------------------------------------------------------------
    # (ZKP_OPT_JOINT_LADDER = 1 is "riders by size", 2 "riders off": no option forces them on, so below 16,384 proofs only the off side is
    #  compared with a forced value; at 16,384 both are)
    dict(row=10, name="riders", const="kRiderLatencyProofs", value=16384, source="fused_flows.h", entry="verify_compact", schedule="latency",
         sizes=(16383, 16384), unit="proofs", key="riders", expect=(0, 1), option=(17, (1, 2)), unreachable=None),
    # Straus lanes per proof: only without window parts, i.e. statements of more than 64 operands (np + nc); w64_statement has 66.  The
    # lanes then rise until a lane holds at most kStrausMaxOpsPerLane = 60 operands, so with K > 64 a proof never gets fewer than 2 lanes
    dict(row=11, name="straus_lanes", const="N >= 16384", value=16384, source="fused_flows.h", entry="verify_batchable_w64", schedule="throughput",
         sizes=(16383, 16384), unit="proofs", key="straus_lanes", expect=(8, 4), option=None, unreachable=None),
    dict(row=11, name="straus_lanes", const="N >= 32768", value=32768, source="fused_flows.h", entry="verify_batchable_w64", schedule="throughput",
         sizes=(32767, 32768), unit="proofs", key="straus_lanes", expect=(4, 2), option=None, unreachable=None),
    dict(row=11, name="straus_lanes", const="N >= 65536", value=65536, source="fused_flows.h", entry="verify_batchable_w64", schedule="throughput",
         sizes=(65535, 65536), unit="proofs", key="straus_lanes", expect=(2, 2), option=None,
         unreachable="the 1 lane this rule picks at 65,536 proofs only applies when window parts are off, i.e. with more than 64 operands per "
                     "proof, and then the kStrausMaxOpsPerLane loop raises it to 2 (more than 60 operands on one lane): no default call sees 1"),
    dict(row=12, name="straus_wins", const="kStrausWinMaxProofs", value=65536, source="fused_flows.h", entry="verify_batchable", schedule="throughput",
         sizes=(65535, 65536), unit="proofs", key="straus_wins", expect=(32, 0), option=None, unreachable=None),
    dict(row=13, name="tr_lanes", const="kVeryWideCallProofs", value=65536, source="zkp_kernels.hip", entry="prove", schedule="throughput",
         sizes=(65535, 65536), unit="proofs", key="tr_lanes", expect=(2, 1), option=(4, (1, 2)), unreachable=None),
    dict(row=14, name="fuse_tt", const="kVeryWideCallProofs", value=65536, source="zkp_kernels.hip", entry="prove", schedule="throughput",
         sizes=(65535, 65536), unit="proofs", key="fuse_tt", expect=(1, 0), option=(8, (0, 1)), unreachable=None),
    dict(row=15, name="tr_steps", const="kVeryWideCallProofs", value=65536, source="fused_flows.h", entry="prove", schedule="latency",
         sizes=(65535, 65536), unit="proofs", key="tr_steps", expect=(1, 0), option=(15, (0, 1)), unreachable=None),
]

# Integer constants of the two sources that are NOT size thresholds of a call, with the reason.  A new k-constant must go into ROWS or here.
NOT_THRESHOLDS = {
    "kMaxEvents": "timing marks per call",
    "kWaveCyclesCap": "capacity of the test-hook cycle recorder",
    "kMergeSeqParts": "per-bucket split of k_pip_bucket_merge: depends on one bucket's part count, not on the call's size, and picks no variant",
    "kMaxBlocks": "grid cap of the one-lane-per-output kernels (larger calls loop in the same kernel)",
    "kWideCallProofs": "declared next to kWideCallTerms and not read anywhere",
    "kStrausMaxLanes": "upper bound of the Straus lanes (the size rule lives in straus_lanes: N >= 16384 / 32768 / 65536)",
    "kStrausMaxOpsPerLane": "LDS bound of one Straus lane: depends on the statement's operand count, not on N",
    "kStrausWinParts": "how many window parts a proof gets once the window split is on (kStrausWinMaxProofs decides that)",
}


# Size rules the source parser does not see (it reads k-constants, and comparisons of n / N / n_terms / n_msm / n_each / total against
# literals of three or more digits or (1u << b)), with what covers them
UNPARSED_RULES = {
    "each_terms_cfg: N >= 2": "verify_batchable without Straus (statements of fewer than 4 operands, or ZKP_OPT_EACH_STRAUS = 0) gives common "
                              "points a comb table from 2 proofs on; a workspace bound only, not a kernel choice",
    "each_terms_cfg: N >= 6": "the same path's comb tables have 16 teeth from 6 proofs on, 4 below; not run at these sizes here",
    "(max_ladder + 255) / 256": "ladder blocks of row 9 (256 lanes per block): exercised by row 9's sizes 65,280 / 65,281",
    "(enc_blocks + ENC_BLOCK - 1) / ENC_BLOCK": "encoder inversion groups: row 2",
}


def row_id(r, size):
    """test id of one row at one size, e.g. "10-riders-16384-latency" """
    return "%s-%s-%d-%s" % (r["row"], r["name"], size, r["schedule"])

//! UNBUILT SOURCE -- see ../../README.md.  Never compiled: no Rust toolchain exists in the build image.
//!
//! `extern "C"` declarations of `include/zkp_mi355x.h` (the HIP engine, libzkp_mi355x.so) and `include/zkp_toolbox.h`
//! (the host toolbox, libzkp_toolbox.so), one declaration per exported symbol, in header order.  Conventions (from the
//! headers): scalars and points are 32-byte strings; buffers are caller-owned and not retained; return 0 = computed,
//! negative = infrastructure failure (NO output may be trusted -- callers must fail closed); `_dev` variants take device
//! pointers and do not synchronise.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct zkp_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zkp_graph {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zkp_statement {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zkp_pipe {
    _private: [u8; 0],
}
#[repr(C)]
pub struct zkp_job {
    _private: [u8; 0],
}

pub const ZKP_OK: c_int = 0;
pub const ZKP_ERR_HIP: c_int = -1;
pub const ZKP_ERR_ARG: c_int = -2;
pub const ZKP_ERR_NO_DEVICE: c_int = -3;
pub const ZKP_ERR_OOM: c_int = -4;
pub const ZKP_VARTIME: c_int = 0; // RistrettoPoint::vartime_multiscalar_mul (verifier.rs:97)
pub const ZKP_CT: c_int = 1; //      RistrettoPoint::multiscalar_mul (prover.rs:94)
pub const ZKP_PT_ADD: c_int = 0; //  zkp_add_points: a + b
pub const ZKP_PT_SUB: c_int = 1; //  zkp_add_points: a - b
pub const ZKP_DLOG_FOUND: u8 = 0; //      zkp_dlog_base status: out[i] B == points[i]
pub const ZKP_DLOG_INVALID: u8 = 1; //    the encoding does not decode
pub const ZKP_DLOG_NOT_FOUND: u8 = 2; //  no logarithm below 2^bits
pub const ZKP_DLOG_SLOTS: u32 = 8; //     zkp_ctx_prepare_dlog_point: slots per context
pub const ZKP_DLOG_SIGNED: c_int = 1; //  zkp_dlog_point flags: k in [-2^(bits-1), 2^(bits-1)) as i64
pub const ZKP_OPT_BATCH_ENCODE_MIN: c_int = 1;
pub const ZKP_OPT_COMB_TEETH: c_int = 2;
pub const ZKP_OPT_CT_SINGLE_USE_TABLES: c_int = 3;
pub const ZKP_OPT_TRANSCRIPT_LANES: c_int = 4;
pub const ZKP_OPT_DEV_OVERLAP: c_int = 5;
pub const ZKP_OPT_GROUPED_COMB: c_int = 6;
pub const ZKP_OPT_TABLES_LANE: c_int = 7;
pub const ZKP_OPT_FUSE_TABLES_TRANSCRIPT: c_int = 8;
pub const ZKP_OPT_CT_LOOKUP: c_int = 9;            // 0 lane crossbar (default), 1 masked scans, 2 LDS rows at the digit's index
pub const ZKP_OPT_CT_MASKED_SCANS: c_int = 9;      // the round-3 name of the same option
pub const ZKP_OPT_EACH_STRAUS: c_int = 10;
pub const ZKP_OPT_LADDER_INTERLEAVE: c_int = 11;
pub const ZKP_OPT_WS_LIMIT_BYTES: c_int = 12;
pub const ZKP_OPT_JOB_DEFER_D2H: c_int = 13;
pub const ZKP_OPT_SYNC_SCHEDULE: c_int = 14;
pub const ZKP_OPT_TRANSCRIPT_STEPS: c_int = 15;
pub const ZKP_OPT_COMB_SPLIT: c_int = 16;
pub const ZKP_OPT_JOINT_LADDER: c_int = 17;
pub const ZKP_JOB_SHARED_TRANSCRIPT: u32 = 1;

pub const ZKP_TB_OK: c_int = 0;
pub const ZKP_TB_VERIFICATION_FAILURE: c_int = 1; // ProofError::VerificationFailure (errors.rs:6)
pub const ZKP_TB_BATCH_SIZE_MISMATCH: c_int = 2; //  ProofError::BatchSizeMismatch   (errors.rs:9)
pub const ZKP_TB_PIPE_FULL: c_int = 3; //             every context of a zkp_pipe has a job in flight
pub const ZKP_TB_BAD_STATEMENT: c_int = -10;
pub const ZKP_TB_INVALID_POINT: c_int = -11;
pub const ZKP_TB_NO_ENTROPY: c_int = -12;
pub const ZKP_TB_BAD_ENCODING: c_int = -13;
pub const ZKP_TRANSCRIPT_BYTES: usize = 208;

/// `zkp_batch_statement`: the statement in point-id form (static ids first, then instance ids).
#[repr(C)]
pub struct zkp_batch_statement {
    pub n_secrets: u32,
    pub n_static: u32,
    pub n_instance: u32,
    pub n_constraints: u32,
    pub cons_lhs: *const u32,
    pub cons_off: *const u32,
    pub cons_sc: *const u32,
    pub cons_pt: *const u32,
}
/// `zkp_fused_statement`: shape + the transcript labels and the allocation order.
#[repr(C)]
pub struct zkp_fused_statement {
    pub shape: zkp_batch_statement,
    pub label: *const c_char,
    pub secret_labels: *const *const c_char,
    pub point_labels: *const *const c_char,
    pub alloc_order: *const u32,
    pub alloc_seq: *const u32, // NULL = define_proof!'s order (all secrets first)
}

extern "C" {
    // ---- zkp_mi355x.h: context ----------------------------------------------------------------------------------
    pub fn zkp_ctx_create(out: *mut *mut zkp_ctx, device_id: c_int) -> c_int;
    pub fn zkp_ctx_destroy(ctx: *mut zkp_ctx);
    pub fn zkp_ctx_set_stream(ctx: *mut zkp_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn zkp_ctx_synchronize(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_last_error() -> *const c_char;
    pub fn zkp_version() -> *const c_char;
    pub fn zkp_ctx_set_option(ctx: *mut zkp_ctx, option: c_int, value: u64) -> c_int;
    pub fn zkp_ctx_capture_begin(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_ctx_capture_end(ctx: *mut zkp_ctx, out: *mut *mut zkp_graph) -> c_int;
    pub fn zkp_ctx_capture_abort(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_graph_launch(graph: *mut zkp_graph, ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_graph_destroy(graph: *mut zkp_graph);
    pub fn zkp_ctx_prepare_fixed_points(ctx: *mut zkp_ctx, n: u32, encodings: *const u8) -> c_int;
    // ---- (1) many small MSMs: prover.rs:94-97 (ZKP_CT), verifier.rs:97-106 (ZKP_VARTIME), + compress (mod.rs:204) ----
    pub fn zkp_msm_many(ctx: *mut zkp_ctx, n_msm: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8,
                        n_points: u32, flags: c_int, out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_msm_many_dev(ctx: *mut zkp_ctx, n_msm: u32, d_off: *const u32, d_scalars: *const u8, d_pidx: *const u32,
                            d_points: *const u8, n_points: u32, n_terms: u32, flags: c_int, d_out: *mut u8, d_status: *mut u8) -> c_int;
    // ---- (2) one large MSM with decode-or-None: verifier.rs:162-166, batch_verifier.rs:219-228 ---------------------
    pub fn zkp_msm_optional(ctx: *mut zkp_ctx, n: u64, scalars: *const u8, points: *const u8, out_point: *mut u8, status: *mut c_int) -> c_int;
    pub fn zkp_msm_optional_dev(ctx: *mut zkp_ctx, n: u64, d_scalars: *const u8, d_points: *const u8, d_out_point: *mut u8,
                                d_status: *mut u32) -> c_int;
    // ---- (2b) batch_verifier.rs:173-234 with the coefficient build on the GPU ----------------------------------------
    pub fn zkp_batch_check(ctx: *mut zkp_ctx, st: *const zkp_batch_statement, n: u32, minus_c: *const u8, responses: *const u8,
                           weights16: *const u8, static_points: *const u8, instance_points: *const u8, commitments: *const u8,
                           out_point: *mut u8, status: *mut c_int, debug_scalars: *mut u8) -> c_int;
    // ---- (2c) fused statement flows ------------------------------------------------------------------------------------
    pub fn zkp_fused_prove(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, secrets: *const u8,
                           inst: *const u8, common: *const u8, entropy: *const u8, challenges: *mut u8, responses: *mut u8,
                           commitments: *mut u8, invalid_point: *mut c_int) -> c_int;
    pub fn zkp_fused_prove_seeded(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, secrets: *const u8, inst: *const u8,
                                  common: *const u8, seed: *const u8, challenges: *mut u8, responses: *mut u8, commitments: *mut u8, invalid_point: *mut c_int) -> c_int;
    pub fn zkp_fused_batch_verify_many_seeded(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n_batches: u32, n_each: u32, transcripts: *mut u8, inst: *const u8,
                                              common: *const u8, commitments: *const u8, responses: *const u8, seed: *const u8, verdicts: *mut c_int) -> c_int;
    pub fn zkp_fused_verify_compact(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, inst: *const u8,
                                    common: *const u8, challenges: *const u8, responses: *const u8, results: *mut u8) -> c_int;
    pub fn zkp_fused_batch_verify(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, inst: *const u8,
                                  common: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                  verdict: *mut c_int, debug_scalars: *mut u8) -> c_int;
    pub fn zkp_fused_batch_verify_many(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n_batches: u32, n_each: u32, transcripts: *mut u8,
                                       inst: *const u8, common: *const u8, commitments: *const u8, responses: *const u8,
                                       weights16: *const u8, verdicts: *mut c_int, debug_scalars: *mut u8) -> c_int;
    pub fn zkp_fused_verify_batchable(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, inst: *const u8,
                                      common: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                      results: *mut u8) -> c_int;
    pub fn zkp_fused_verify_batchable_coeffs(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8,
                                             inst: *const u8, common: *const u8, commitments: *const u8, responses: *const u8,
                                             weights16: *const u8, results: *mut u8, debug_scalars: *mut u8) -> c_int;
    pub fn zkp_fused_prove_dev(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, strobe_pos: u32, d_transcripts: *mut u8,
                               d_secrets: *const u8, d_table: *const u8, d_entropy: *const u8, d_challenges: *mut u8,
                               d_responses: *mut u8, d_commitments: *mut u8, d_status: *mut u8) -> c_int;
    pub fn zkp_fused_verify_compact_dev(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, strobe_pos: u32,
                                        d_transcripts: *mut u8, d_table: *const u8, d_challenges: *const u8, d_responses: *const u8,
                                        d_results: *mut u8) -> c_int;
    pub fn zkp_fused_verify_batchable_dev(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, strobe_pos: u32,
                                          d_transcripts: *mut u8, d_table: *const u8, d_responses: *const u8,
                                          d_weights16: *const u8, d_results: *mut u8) -> c_int;
    pub fn zkp_fused_batch_verify_dev(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, strobe_pos: u32,
                                      d_transcripts: *mut u8, d_points: *mut u8, d_commitments: *const u8, d_responses: *const u8,
                                      d_weights16: *const u8, d_out_point: *mut u8, d_status: *mut u32) -> c_int;
    pub fn zkp_fused_batch_verify_many_dev(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n_batches: u32, n_each: u32, strobe_pos: u32,
                                           d_transcripts: *mut u8, d_points: *mut u8, d_commitments: *const u8, d_responses: *const u8,
                                           d_weights16: *const u8, d_out_points: *mut u8, d_status: *mut u32) -> c_int;
    // ---- (2d) the fused flows on host buffers as asynchronous jobs (one per context), pinned memory, device ChaCha20 ------
    pub fn zkp_fused_prove_submit(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, flags: u32, transcripts: *const u8, secrets: *const u8,
                                  inst: *const u8, inst_stride: u32, common: *const u8, entropy: *const u8, rng_seed: *const u8,
                                  transcripts_out: *mut u8, challenges: *mut u8, responses: *mut u8, commitments: *mut u8,
                                  invalid_point: *mut c_int) -> c_int;
    pub fn zkp_fused_verify_compact_submit(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, flags: u32, transcripts: *const u8,
                                           inst: *const u8, inst_stride: u32, common: *const u8, challenges: *const u8, responses: *const u8,
                                           transcripts_out: *mut u8, results: *mut u8) -> c_int;
    pub fn zkp_fused_batch_verify_many_submit(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n_batches: u32, n_each: u32, flags: u32,
                                              transcripts: *const u8, inst: *const u8, inst_stride: u32, common: *const u8,
                                              commitments: *const u8, responses: *const u8, weights16: *const u8, weights_stride: u32,
                                              rng_seed: *const u8, transcripts_out: *mut u8, verdicts: *mut c_int) -> c_int;
    pub fn zkp_fused_verify_batchable_submit(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, flags: u32, transcripts: *const u8,
                                             inst: *const u8, inst_stride: u32, common: *const u8, commitments: *const u8,
                                             responses: *const u8, weights16: *const u8, rng_seed: *const u8, transcripts_out: *mut u8,
                                             results: *mut u8) -> c_int;
    pub fn zkp_ctx_job_wait(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_ctx_job_poll(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_ctx_job_pending(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_ctx_job_discard(ctx: *mut zkp_ctx) -> c_int;
    pub fn zkp_ctx_job_timing(ctx: *mut zkp_ctx, ms: *mut f32) -> c_int;
    pub fn zkp_host_alloc(out: *mut *mut c_void, bytes: usize) -> c_int;
    pub fn zkp_host_alloc_on(out: *mut *mut c_void, bytes: usize, device: c_int) -> c_int;
    pub fn zkp_host_numa_node(device: c_int) -> c_int;
    pub fn zkp_host_node_of(p: *const c_void) -> c_int;
    pub fn zkp_host_free(p: *mut c_void);
    pub fn zkp_host_register(p: *mut c_void, bytes: usize) -> c_int;
    pub fn zkp_host_unregister(p: *mut c_void) -> c_int;
    pub fn zkp_host_is_pinned(p: *const c_void) -> c_int;
    pub fn zkp_chacha20_fill_dev(ctx: *mut zkp_ctx, key: *const u8, nonce: u64, first_block: u64, d_out: *mut u8, bytes: usize) -> c_int;
    // ---- (3), (4) stand-alone codec: verifier.rs:87-92, mod.rs:180 -------------------------------------------------------
    pub fn zkp_decode_check(ctx: *mut zkp_ctx, n: u64, points: *const u8, status: *mut u8, xyzt: *mut u8) -> c_int;
    pub fn zkp_encode_many(ctx: *mut zkp_ctx, n: u64, xyzt: *const u8, out: *mut u8) -> c_int;
    // ---- (5) hash to the group: RistrettoPoint::from_uniform_bytes (RFC 9496 4.3.4), sig_and_vrf_example.rs:36-40 --------
    pub fn zkp_from_uniform_bytes(ctx: *mut zkp_ctx, n: u64, input: *const u8, out: *mut u8) -> c_int;
    pub fn zkp_from_uniform_bytes_dev(ctx: *mut zkp_ctx, n: u64, d_in: *const u8, d_out: *mut u8) -> c_int;
    pub fn zkp_fused_hash_to_group(ctx: *mut zkp_ctx, n: u32, transcripts: *mut u8, label: *const c_char, out: *mut u8) -> c_int;
    // ragged batches: transcripts at different STROBE positions (synchronous, host pointers; aligned batches accepted too)
    pub fn zkp_fused_hash_to_group_ragged(ctx: *mut zkp_ctx, n: u32, transcripts: *mut u8, label: *const c_char, out: *mut u8) -> c_int;
    pub fn zkp_fused_prove_ragged(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, secrets: *const u8, inst: *const u8,
                                  common: *const u8, entropy: *const u8, seed: *const u8, challenges: *mut u8, responses: *mut u8, commitments: *mut u8,
                                  invalid_point: *mut c_int) -> c_int;
    pub fn zkp_fused_verify_compact_ragged(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, inst: *const u8,
                                           common: *const u8, challenges: *const u8, responses: *const u8, results: *mut u8) -> c_int;
    pub fn zkp_fused_verify_batchable_ragged(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n: u32, transcripts: *mut u8, inst: *const u8,
                                             common: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8, results: *mut u8) -> c_int;
    pub fn zkp_fused_batch_verify_many_ragged(ctx: *mut zkp_ctx, st: *const zkp_fused_statement, n_batches: u32, n_each: u32, transcripts: *mut u8,
                                              inst: *const u8, common: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                              seed: *const u8, verdicts: *mut c_int) -> c_int;
    // hash_from_bytes::<Sha512> over a CSR batch of messages (zkp.rs:34): SHA-512, then from_uniform_bytes
    pub fn zkp_hash_from_bytes_sha512(ctx: *mut zkp_ctx, n: u64, msgs: *const u8, offsets: *const u64, out: *mut u8) -> c_int;
    pub fn zkp_hash_from_bytes_sha512_dev(ctx: *mut zkp_ctx, n: u64, d_msgs: *const u8, msgs_len: u64, d_offsets: *const u64, d_out: *mut u8) -> c_int;
    // scalars mod l, batched (Scalar::invert, from_bytes_mod_order_wide, a * b + c, Scalar::random, hash_from_bytes::<Sha512>)
    pub fn zkp_sc_invert(ctx: *mut zkp_ctx, n: u64, input: *const u8, out: *mut u8) -> c_int;
    pub fn zkp_sc_invert_dev(ctx: *mut zkp_ctx, n: u64, d_in: *const u8, d_out: *mut u8) -> c_int;
    pub fn zkp_sc_from_wide(ctx: *mut zkp_ctx, n: u64, input: *const u8, out: *mut u8) -> c_int;
    pub fn zkp_sc_from_wide_dev(ctx: *mut zkp_ctx, n: u64, d_in: *const u8, d_out: *mut u8) -> c_int;
    pub fn zkp_sc_muladd(ctx: *mut zkp_ctx, n: u64, a: *const u8, a_stride: u32, b: *const u8, b_stride: u32, c: *const u8, c_stride: u32,
                         out: *mut u8) -> c_int;
    pub fn zkp_sc_muladd_dev(ctx: *mut zkp_ctx, n: u64, d_a: *const u8, a_stride: u32, d_b: *const u8, b_stride: u32, d_c: *const u8, c_stride: u32,
                             d_out: *mut u8) -> c_int;
    pub fn zkp_sc_random(ctx: *mut zkp_ctx, n: u64, key: *const u8, nonce: u64, out: *mut u8) -> c_int;
    pub fn zkp_sc_random_dev(ctx: *mut zkp_ctx, n: u64, key: *const u8, nonce: u64, d_out: *mut u8) -> c_int;
    pub fn zkp_sc_hash_from_bytes_sha512(ctx: *mut zkp_ctx, n: u64, msgs: *const u8, offsets: *const u64, out: *mut u8) -> c_int;
    pub fn zkp_sc_hash_from_bytes_sha512_dev(ctx: *mut zkp_ctx, n: u64, d_msgs: *const u8, msgs_len: u64, d_offsets: *const u64, d_out: *mut u8) -> c_int;
    // (8) Scalar * basepoint (`&sk * &RISTRETTO_BASEPOINT_TABLE`) and Scalar * point (`&H * &x`), batched, each with its compress()
    pub fn zkp_mul_base(ctx: *mut zkp_ctx, n: u64, scalars: *const u8, out: *mut u8) -> c_int;
    pub fn zkp_mul_base_dev(ctx: *mut zkp_ctx, n: u64, d_scalars: *const u8, d_out: *mut u8) -> c_int;
    pub fn zkp_mul_points(ctx: *mut zkp_ctx, n: u64, scalars: *const u8, s_stride: u32, points: *const u8, p_stride: u32, flags: c_int, out: *mut u8,
                          status: *mut u8) -> c_int;
    pub fn zkp_mul_points_dev(ctx: *mut zkp_ctx, n: u64, d_scalars: *const u8, s_stride: u32, d_points: *const u8, p_stride: u32, flags: c_int,
                              d_out: *mut u8, d_status: *mut u8) -> c_int;
    // (9) RistrettoPoint sums: pairs (op = ZKP_PT_ADD / ZKP_PT_SUB) and CSR segments, each with its compress()
    pub fn zkp_add_points(ctx: *mut zkp_ctx, n: u64, a: *const u8, a_stride: u32, b: *const u8, b_stride: u32, op: c_int, out: *mut u8,
                          status: *mut u8) -> c_int;
    pub fn zkp_add_points_dev(ctx: *mut zkp_ctx, n: u64, d_a: *const u8, a_stride: u32, d_b: *const u8, b_stride: u32, op: c_int, d_out: *mut u8,
                              d_status: *mut u8) -> c_int;
    pub fn zkp_sum_points(ctx: *mut zkp_ctx, n_sums: u32, off: *const u32, pidx: *const u32, neg: *const u8, points: *const u8, n_points: u32,
                          out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_sum_points_dev(ctx: *mut zkp_ctx, n_sums: u32, d_off: *const u32, d_pidx: *const u32, d_neg: *const u8, d_points: *const u8,
                              n_points: u32, n_terms: u32, d_out: *mut u8, d_status: *mut u8) -> c_int;
    pub fn zkp_sum_points_group() -> u32;
    // (11) multiscalar sums with long segments: zkp_msm_many's results, the term axis folded in the levels of zkp_sum_points
    pub fn zkp_msm_segments(ctx: *mut zkp_ctx, n_msm: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8, n_points: u32,
                            flags: c_int, out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_msm_segments_dev(ctx: *mut zkp_ctx, n_msm: u32, d_off: *const u32, d_scalars: *const u8, d_pidx: *const u32, d_points: *const u8,
                                n_points: u32, n_terms: u32, flags: c_int, d_out: *mut u8, d_status: *mut u8) -> c_int;
    // (14) many variable-time multiscalar sums with long segments by the bucket method (no flags: variable time by definition); the segment length
    // above which bucket runs are used
    pub fn zkp_msm_optional_many(ctx: *mut zkp_ctx, n_seg: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8, n_points: u32,
                                 out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_msm_optional_many_dev(ctx: *mut zkp_ctx, n_seg: u32, d_off: *const u32, d_scalars: *const u8, d_pidx: *const u32, d_points: *const u8,
                                     n_points: u32, n_terms: u32, max_seg: u32, d_out: *mut u8, d_status: *mut u8) -> c_int;
    pub fn zkp_msm_optional_many_min_segment() -> u32;
    // (12) segmented scalar sums, products and dot products (op: 0 sum, 1 product, 2 dot); the work unit's size and the number of fold launches
    pub fn zkp_sc_reduce(ctx: *mut zkp_ctx, op: c_int, n_out: u32, off: *const u32, a: *const u8, n_a: u32, aidx: *const u32, b: *const u8, n_b: u32,
                         bidx: *const u32, out: *mut u8) -> c_int;
    pub fn zkp_sc_reduce_dev(ctx: *mut zkp_ctx, op: c_int, n_out: u32, d_off: *const u32, d_a: *const u8, n_a: u32, d_aidx: *const u32, d_b: *const u8,
                             n_b: u32, d_bidx: *const u32, n_terms: u32, d_out: *mut u8) -> c_int;
    pub fn zkp_sc_reduce_group() -> u32;
    pub fn zkp_sc_reduce_levels(n_terms: u32) -> u32;
    // (13) segmented prefix sums and products of scalars, running sums of points (mode: 0 inclusive, 1 exclusive): one row per term
    pub fn zkp_sc_scan(ctx: *mut zkp_ctx, op: c_int, mode: c_int, n_seg: u32, off: *const u32, a: *const u8, n_a: u32, aidx: *const u32, out: *mut u8) -> c_int;
    pub fn zkp_sc_scan_dev(ctx: *mut zkp_ctx, op: c_int, mode: c_int, n_seg: u32, d_off: *const u32, d_a: *const u8, n_a: u32, d_aidx: *const u32,
                           n_terms: u32, d_out: *mut u8) -> c_int;
    pub fn zkp_sc_scan_group() -> u32;
    pub fn zkp_sc_scan_launches(n_terms: u32) -> u32;
    pub fn zkp_scan_points(ctx: *mut zkp_ctx, mode: c_int, n_seg: u32, off: *const u32, pidx: *const u32, neg: *const u8, points: *const u8, n_points: u32,
                           out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_scan_points_dev(ctx: *mut zkp_ctx, mode: c_int, n_seg: u32, d_off: *const u32, d_pidx: *const u32, d_neg: *const u8, d_points: *const u8,
                               n_points: u32, n_terms: u32, d_out: *mut u8, d_status: *mut u8) -> c_int;
    pub fn zkp_scan_points_group() -> u32;
    pub fn zkp_scan_points_launches(n_terms: u32) -> u32;
    // (10) bounded discrete logarithms to the basepoint (variable time by nature): the context's baby-step table and the search
    pub fn zkp_ctx_prepare_dlog(ctx: *mut zkp_ctx, baby_bits: u32) -> c_int;
    pub fn zkp_dlog_baby_bits(ctx: *mut zkp_ctx) -> u32;
    pub fn zkp_dlog_base(ctx: *mut zkp_ctx, n: u64, points: *const u8, bits: u32, out: *mut u64, status: *mut u8) -> c_int;
    pub fn zkp_dlog_base_dev(ctx: *mut zkp_ctx, n: u64, d_points: *const u8, bits: u32, d_out: *mut u64, d_status: *mut u8) -> c_int;
    pub fn zkp_dlog_group() -> u32;
    pub fn zkp_dlog_chunk() -> u32;
    pub fn zkp_dlog_slice_chunks(n: u64) -> u32;
    pub fn zkp_ctx_prepare_dlog_point(ctx: *mut zkp_ctx, slot: u32, base: *const u8, baby_bits: u32) -> c_int;
    pub fn zkp_ctx_release_dlog_point(ctx: *mut zkp_ctx, slot: u32) -> c_int;
    pub fn zkp_dlog_point_baby_bits(ctx: *mut zkp_ctx, slot: u32) -> u32;
    pub fn zkp_dlog_point_base(ctx: *mut zkp_ctx, slot: u32, out: *mut u8) -> c_int;
    pub fn zkp_dlog_point_find(ctx: *mut zkp_ctx, base: *const u8) -> c_int;
    pub fn zkp_dlog_point_last_use(ctx: *mut zkp_ctx, slot: u32) -> usize;
    pub fn zkp_dlog_point(ctx: *mut zkp_ctx, slot: u32, n: u64, points: *const u8, bits: u32, flags: c_int, out: *mut u64, status: *mut u8) -> c_int;
    pub fn zkp_dlog_point_dev(ctx: *mut zkp_ctx, slot: u32, n: u64, d_points: *const u8, bits: u32, flags: c_int, d_out: *mut u64, d_status: *mut u8) -> c_int;
    pub fn zkp_dlog_slice_order(n_slices: u64, flags: c_int, i: u64) -> usize;
    pub fn zkp_dlog_slice_chunks_signed(n: u64) -> u32;
    // (7) Merlin operations on N transcripts at any mix of positions
    pub fn zkp_transcripts_append_message(ctx: *mut zkp_ctx, n: u32, shared_initial: c_int, ts: *mut u8, label: *const c_char, msgs: *const u8,
                                          offsets: *const u64) -> c_int;
    pub fn zkp_transcripts_append_message_dev(ctx: *mut zkp_ctx, n: u32, shared_initial: c_int, d_ts_in: *const u8, d_ts_out: *mut u8, label: *const c_char,
                                              d_msgs: *const u8, msgs_len: u64, d_offsets: *const u64) -> c_int;
    pub fn zkp_transcripts_challenge_bytes(ctx: *mut zkp_ctx, n: u32, ts: *mut u8, label: *const c_char, len: u32, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_challenge_bytes_dev(ctx: *mut zkp_ctx, n: u32, d_ts: *mut u8, label: *const c_char, len: u32, d_out: *mut u8) -> c_int;
    pub fn zkp_strobe_pos_after_append(strobe_pos: u32, label_len: u64, msg_len: u64) -> u32;
    pub fn zkp_transcripts_witness_rng(ctx: *mut zkp_ctx, n: u32, ts: *const u8, label: *const c_char, m: u32, wlen: u32, witnesses: *const u8, entropy: *const u8,
                                       mode: c_int, count: u32, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_witness_rng_dev(ctx: *mut zkp_ctx, n: u32, d_ts: *const u8, label: *const c_char, m: u32, wlen: u32, d_witnesses: *const u8,
                                           d_entropy: *const u8, mode: c_int, count: u32, d_out: *mut u8) -> c_int;
    pub fn zkp_transcripts_challenge_scalars(ctx: *mut zkp_ctx, n: u32, ts: *mut u8, label: *const c_char, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_challenge_scalars_dev(ctx: *mut zkp_ctx, n: u32, d_ts: *mut u8, label: *const c_char, d_out: *mut u8) -> c_int;
    pub fn zkp_transcripts_append_points(ctx: *mut zkp_ctx, n: u32, ts: *mut u8, kind: *const c_char, var_label: *const c_char, points: *const u8,
                                         validate: c_int, status: *mut u8) -> c_int;
    pub fn zkp_transcripts_append_points_dev(ctx: *mut zkp_ctx, n: u32, d_ts: *mut u8, kind: *const c_char, var_label: *const c_char, d_points: *const u8,
                                             validate: c_int, d_status: *mut u8) -> c_int;
    pub fn zkp_ctx_last_timing(ctx: *mut zkp_ctx, kernel_ms: *mut f32, total_ms: *mut f32) -> c_int;
    pub fn zkp_ctx_last_kernels(ctx: *mut zkp_ctx, kind: c_int, buf: *mut c_char, cap: usize) -> c_int;
    pub fn zkp_ctx_set_profiling(ctx: *mut zkp_ctx, enabled: c_int) -> c_int;

    // ---- zkp_toolbox.h: Merlin transcripts, scalars ---------------------------------------------------------------------
    pub fn zkp_transcript_init(t: *mut u8, label: *const u8, label_len: usize);
    pub fn zkp_transcript_append_message(t: *mut u8, label: *const c_char, msg: *const u8, len: usize) -> c_int;
    pub fn zkp_transcript_challenge_bytes(t: *mut u8, label: *const c_char, out: *mut u8, len: usize) -> c_int;
    pub fn zkp_transcripts_append_message_batch(ts: *mut u8, n: u32, shared_initial: c_int, label: *const c_char, msgs: *const u8, offsets: *const u64,
                                                n_threads: c_int) -> c_int;
    pub fn zkp_transcripts_append_message_batch_ctx(ctx: *mut zkp_ctx, ts: *mut u8, n: u32, shared_initial: c_int, label: *const c_char, msgs: *const u8,
                                                    offsets: *const u64, n_threads: c_int) -> c_int;
    pub fn zkp_transcripts_challenge_bytes_batch(ctx: *mut zkp_ctx, ts: *mut u8, n: u32, label: *const c_char, len: u32, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_witness_rng_batch(ctx: *mut zkp_ctx, ts: *const u8, n: u32, label: *const c_char, m: u32, wlen: u32, witnesses: *const u8,
                                             entropy: *const u8, mode: c_int, count: u32, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_challenge_scalars_batch(ctx: *mut zkp_ctx, ts: *mut u8, n: u32, label: *const c_char, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_transcripts_append_points_batch(ctx: *mut zkp_ctx, ts: *mut u8, n: u32, kind: *const c_char, var_label: *const c_char, points: *const u8,
                                               validate: c_int, n_threads: c_int, status: *mut u8) -> c_int;
    pub fn zkp_toolbox_set_witness_rng_min_batch(n: u32);
    pub fn zkp_toolbox_get_witness_rng_min_batch() -> u32;
    pub fn zkp_toolbox_set_challenge_scalars_min_batch(n: u32);
    pub fn zkp_toolbox_get_challenge_scalars_min_batch() -> u32;
    pub fn zkp_toolbox_set_append_points_min_batch(n: u32);
    pub fn zkp_toolbox_get_append_points_min_batch() -> u32;
    pub fn zkp_scalar_from_wide(out: *mut u8, input: *const u8);
    pub fn zkp_scalar_muladd(out: *mut u8, a: *const u8, b: *const u8, c: *const u8);
    pub fn zkp_scalar_neg(out: *mut u8, a: *const u8);
    // ---- statements (what define_proof! fixes: macros.rs:124-138, 159-170) ----------------------------------------------
    pub fn zkp_statement_new(proof_label: *const c_char) -> *mut zkp_statement;
    pub fn zkp_statement_free(st: *mut zkp_statement);
    pub fn zkp_statement_add_secret(st: *mut zkp_statement, name: *const c_char) -> c_int;
    pub fn zkp_statement_add_point(st: *mut zkp_statement, name: *const c_char, is_common: c_int) -> c_int;
    pub fn zkp_statement_constrain(st: *mut zkp_statement, lhs_point: u32, n_terms: u32, secrets: *const u32, points: *const u32) -> c_int;
    pub fn zkp_statement_num_secrets(st: *const zkp_statement) -> u32;
    pub fn zkp_statement_num_instance(st: *const zkp_statement) -> u32;
    pub fn zkp_statement_num_common(st: *const zkp_statement) -> u32;
    pub fn zkp_statement_num_constraints(st: *const zkp_statement) -> u32;
    pub fn zkp_statement_num_terms(st: *const zkp_statement) -> u32;
    // ---- batched flows -------------------------------------------------------------------------------------------------
    pub fn zkp_prove_batch(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, transcripts: *mut u8, secrets: *const u8,
                           inst_points: *const u8, common_points: *const u8, entropy: *const u8, n_threads: c_int,
                           challenges: *mut u8, responses: *mut u8, commitments: *mut u8) -> c_int;
    pub fn zkp_verify_compact_batch(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, transcripts: *mut u8, inst_points: *const u8,
                                    common_points: *const u8, challenges: *const u8, responses: *const u8, n_threads: c_int,
                                    results: *mut u8) -> c_int;
    pub fn zkp_verify_batchable_each(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, transcripts: *mut u8, inst_points: *const u8,
                                     common_points: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                     n_threads: c_int, results: *mut u8) -> c_int;
    pub fn zkp_batch_verify(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8,
                            inst_points: *const u8, common_points: *const u8, commitments: *const u8, responses: *const u8,
                            weights16: *const u8, n_threads: c_int) -> c_int;
    pub fn zkp_batch_verify_coeffs(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8,
                                   inst_points: *const u8, common_points: *const u8, commitments: *const u8, responses: *const u8,
                                   weights16: *const u8, n_threads: c_int, coeffs: *mut u8) -> c_int;
    pub fn zkp_batch_verify_many(ctx: *mut zkp_ctx, st: *const zkp_statement, n_batches: u32, n_each: u32, n_transcripts: u32,
                                 transcripts: *mut u8, inst_points: *const u8, common_points: *const u8, commitments: *const u8,
                                 responses: *const u8, weights16: *const u8, n_threads: c_int, verdicts: *mut c_int) -> c_int;
    pub fn zkp_batch_verify_locate(ctx: *mut zkp_ctx, st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8,
                                   inst_points: *const u8, common_points: *const u8, commitments: *const u8, responses: *const u8,
                                   weights16: *const u8, n_threads: c_int, results: *mut u8) -> c_int;
    // ---- pipelines and device groups: contexts over one or several GPUs, asynchronous jobs, sharded synchronous calls ------
    pub fn zkp_pipe_create(out: *mut *mut zkp_pipe, device_ids: *const c_int, n_devices: c_int, contexts_per_device: c_int) -> c_int;
    pub fn zkp_pipe_destroy(pipe: *mut zkp_pipe);
    pub fn zkp_pipe_num_contexts(pipe: *const zkp_pipe) -> c_int;
    pub fn zkp_pipe_num_devices(pipe: *const zkp_pipe) -> c_int;
    pub fn zkp_pipe_context(pipe: *mut zkp_pipe, i: c_int) -> *mut zkp_ctx;
    pub fn zkp_pipe_context_device(pipe: *const zkp_pipe, i: c_int) -> c_int;
    pub fn zkp_pipe_shard_plan(n_items: u32, unit: u32, n_contexts: u32, fused_min_batch: u32, lo: *mut u32, hi: *mut u32) -> u32;
    pub fn zkp_pipe_jobs_in_flight(pipe: *const zkp_pipe) -> c_int;
    pub fn zkp_pipe_set_submit_threads(pipe: *mut zkp_pipe, on: c_int) -> c_int;
    pub fn zkp_pipe_last_error(pipe: *const zkp_pipe) -> *const c_char;
    pub fn zkp_prove_batch_submit(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, flags: u32, transcripts: *const u8, secrets: *const u8,
                                  inst_points: *const u8, inst_stride: u32, common_points: *const u8, entropy: *const u8,
                                  transcripts_out: *mut u8, challenges: *mut u8, responses: *mut u8, commitments: *mut u8,
                                  job: *mut *mut zkp_job) -> c_int;
    pub fn zkp_verify_compact_batch_submit(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, flags: u32, transcripts: *const u8,
                                           inst_points: *const u8, inst_stride: u32, common_points: *const u8, challenges: *const u8,
                                           responses: *const u8, transcripts_out: *mut u8, results: *mut u8, job: *mut *mut zkp_job) -> c_int;
    pub fn zkp_verify_batchable_each_submit(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, flags: u32, transcripts: *const u8,
                                            inst_points: *const u8, inst_stride: u32, common_points: *const u8, commitments: *const u8,
                                            responses: *const u8, weights16: *const u8, transcripts_out: *mut u8, results: *mut u8,
                                            job: *mut *mut zkp_job) -> c_int;
    pub fn zkp_batch_verify_many_submit(pipe: *mut zkp_pipe, st: *const zkp_statement, n_batches: u32, n_each: u32, flags: u32,
                                        transcripts: *const u8, inst_points: *const u8, inst_stride: u32, common_points: *const u8,
                                        commitments: *const u8, responses: *const u8, weights16: *const u8, weights_stride: u32,
                                        transcripts_out: *mut u8, verdicts: *mut c_int, job: *mut *mut zkp_job) -> c_int;
    pub fn zkp_job_context_index(job: *const zkp_job) -> c_int;
    pub fn zkp_job_done(job: *const zkp_job) -> c_int;
    pub fn zkp_job_wait(job: *mut zkp_job) -> c_int;
    pub fn zkp_pipe_prove_batch(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, transcripts: *mut u8, secrets: *const u8,
                                inst_points: *const u8, common_points: *const u8, entropy: *const u8, challenges: *mut u8,
                                responses: *mut u8, commitments: *mut u8) -> c_int;
    pub fn zkp_pipe_verify_compact_batch(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, transcripts: *mut u8, inst_points: *const u8,
                                         common_points: *const u8, challenges: *const u8, responses: *const u8, results: *mut u8) -> c_int;
    pub fn zkp_pipe_verify_batchable_each(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, transcripts: *mut u8, inst_points: *const u8,
                                          common_points: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                          results: *mut u8) -> c_int;
    pub fn zkp_pipe_batch_verify(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8,
                                 inst_points: *const u8, common_points: *const u8, commitments: *const u8, responses: *const u8,
                                 weights16: *const u8) -> c_int;
    pub fn zkp_pipe_batch_verify_many(pipe: *mut zkp_pipe, st: *const zkp_statement, n_batches: u32, n_each: u32, n_transcripts: u32,
                                      transcripts: *mut u8, inst_points: *const u8, common_points: *const u8, commitments: *const u8,
                                      responses: *const u8, weights16: *const u8, verdicts: *mut c_int) -> c_int;
    pub fn zkp_pipe_batch_verify_locate(pipe: *mut zkp_pipe, st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8,
                                        inst_points: *const u8, common_points: *const u8, commitments: *const u8, responses: *const u8,
                                        weights16: *const u8, results: *mut u8) -> c_int;
    pub fn zkp_toolbox_set_host_max_terms(n: u32);
    pub fn zkp_toolbox_get_host_max_terms() -> u32;
    pub fn zkp_toolbox_set_fused_min_batch(n: u32);
    pub fn zkp_toolbox_get_fused_min_batch() -> u32;
    // hash to the group on the host backend (ctx NULL or n <= host_max_terms) or the device
    pub fn zkp_from_uniform_bytes_batch(ctx: *mut zkp_ctx, n: u64, input: *const u8, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_hash_to_group_batch(ctx: *mut zkp_ctx, n: u32, transcripts: *mut u8, label: *const c_char, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_hash_from_bytes_sha512_batch(ctx: *mut zkp_ctx, n: u64, msgs: *const u8, offsets: *const u64, n_threads: c_int, out: *mut u8) -> c_int;
    // scalars mod l on the host backend (ctx NULL or n <= host_max_terms) or the device
    pub fn zkp_scalar_invert_batch(ctx: *mut zkp_ctx, n: u64, input: *const u8, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_scalar_from_wide_batch(ctx: *mut zkp_ctx, n: u64, input: *const u8, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_scalar_muladd_batch(ctx: *mut zkp_ctx, n: u64, a: *const u8, a_stride: u32, b: *const u8, b_stride: u32, c: *const u8, c_stride: u32,
                                   n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_scalar_hash_from_bytes_sha512_batch(ctx: *mut zkp_ctx, n: u64, msgs: *const u8, offsets: *const u64, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_scalar_random_batch(ctx: *mut zkp_ctx, n: u64, key: *const u8, nonce: u64, n_threads: c_int, out: *mut u8) -> c_int;
    // Scalar * basepoint, Scalar * point and multiscalar products behind the same routing
    pub fn zkp_basepoint_mul_batch(ctx: *mut zkp_ctx, n: u64, scalars: *const u8, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_point_mul_batch(ctx: *mut zkp_ctx, n: u64, scalars: *const u8, s_stride: u32, points: *const u8, p_stride: u32, flags: c_int,
                               n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_multiscalar_mul_batch(ctx: *mut zkp_ctx, n_msm: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8,
                                     n_points: u32, flags: c_int, n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    // RistrettoPoint sums behind the same routing
    pub fn zkp_point_add_batch(ctx: *mut zkp_ctx, n: u64, a: *const u8, a_stride: u32, b: *const u8, b_stride: u32, op: c_int, n_threads: c_int,
                               out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_point_sum_batch(ctx: *mut zkp_ctx, n_sums: u32, off: *const u32, pidx: *const u32, neg: *const u8, points: *const u8, n_points: u32,
                               n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    // multiscalar sums routed by size and by the longest segment (host threads / zkp_msm_many / zkp_msm_segments) and the segment threshold
    pub fn zkp_multiscalar_sum_batch(ctx: *mut zkp_ctx, n_msm: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8,
                                     n_points: u32, flags: c_int, n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    // segmented scalar sums, products and dot products routed by the number of terms (host threads / zkp_sc_reduce) and the per-op threshold
    pub fn zkp_scalar_reduce_batch(ctx: *mut zkp_ctx, op: c_int, n_out: u32, off: *const u32, a: *const u8, n_a: u32, aidx: *const u32, b: *const u8,
                                   n_b: u32, bidx: *const u32, n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_toolbox_set_scalar_reduce_min_terms(op: c_int, n: u64);
    pub fn zkp_toolbox_get_scalar_reduce_min_terms(op: c_int) -> usize;
    // segmented prefix sums and products of scalars and running sums of points, routed by the number of terms (host threads / zkp_sc_scan, zkp_scan_points)
    pub fn zkp_scalar_scan_batch(ctx: *mut zkp_ctx, op: c_int, mode: c_int, n_seg: u32, off: *const u32, a: *const u8, n_a: u32, aidx: *const u32,
                                 n_threads: c_int, out: *mut u8) -> c_int;
    pub fn zkp_point_scan_batch(ctx: *mut zkp_ctx, mode: c_int, n_seg: u32, off: *const u32, pidx: *const u32, neg: *const u8, points: *const u8,
                                n_points: u32, n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_toolbox_set_scalar_scan_min_terms(op: c_int, n: u64);
    pub fn zkp_toolbox_get_scalar_scan_min_terms(op: c_int) -> usize;
    pub fn zkp_toolbox_set_point_scan_min_terms(n: u64);
    pub fn zkp_toolbox_get_point_scan_min_terms() -> usize;
    pub fn zkp_toolbox_set_msm_fold_min_segment(n: u32);
    pub fn zkp_toolbox_get_msm_fold_min_segment() -> u32;
    // the same sums, variable time, routed by size and by the longest segment (host threads / zkp_multiscalar_sum_batch's route / zkp_msm_optional_many)
    pub fn zkp_multiscalar_optional_batch(ctx: *mut zkp_ctx, n_seg: u32, off: *const u32, scalars: *const u8, pidx: *const u32, points: *const u8,
                                          n_points: u32, n_threads: c_int, out: *mut u8, status: *mut u8) -> c_int;
    pub fn zkp_toolbox_set_msm_bucket_min_segment(n: u32);
    pub fn zkp_toolbox_get_msm_bucket_min_segment() -> u32;
    // bounded discrete logarithms to the basepoint behind the same routing; the host table's size and the routing threshold
    pub fn zkp_basepoint_dlog_batch(ctx: *mut zkp_ctx, n: u64, points: *const u8, bits: u32, out: *mut u64, status: *mut u8, n_threads: c_int) -> c_int;
    pub fn zkp_point_dlog_batch(ctx: *mut zkp_ctx, base: *const u8, n: u64, points: *const u8, bits: u32, flags: c_int, out: *mut u64, status: *mut u8, n_threads: c_int) -> c_int;
    pub fn zkp_toolbox_set_dlog_baby_bits(baby_bits: u32) -> c_int;
    pub fn zkp_toolbox_get_dlog_baby_bits() -> u32;
    pub fn zkp_toolbox_set_dlog_host_max_steps(steps: u32);
    pub fn zkp_toolbox_get_dlog_host_max_steps() -> u32;
    pub fn zkp_chacha20_block(key: *const u8, counter: u64, nonce: u64, out: *mut u8);
    // ---- proof wire format (proofs.rs:14-32 under bincode 1.x) ------------------------------------------------------------
    pub fn zkp_proof_compact_size(m: u32) -> usize;
    pub fn zkp_proof_batchable_size(nc: u32, m: u32) -> usize;
    pub fn zkp_proof_compact_encode(challenge: *const u8, responses: *const u8, m: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn zkp_proof_compact_decode(input: *const u8, len: usize, challenge: *mut u8, responses: *mut u8, max_m: u32, m: *mut u32,
                                    consumed: *mut usize) -> c_int;
    pub fn zkp_proof_batchable_encode(commitments: *const u8, nc: u32, responses: *const u8, m: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn zkp_proof_batchable_decode(input: *const u8, len: usize, commitments: *mut u8, max_nc: u32, nc: *mut u32, responses: *mut u8,
                                      max_m: u32, m: *mut u32, consumed: *mut usize) -> c_int;
    // ---- host-only halves (tests) -----------------------------------------------------------------------------------------
    pub fn zkp_batch_verify_build(st: *const zkp_statement, n: u32, n_transcripts: u32, transcripts: *mut u8, inst_points: *const u8,
                                  common_points: *const u8, commitments: *const u8, responses: *const u8, weights16: *const u8,
                                  n_threads: c_int, msm_scalars: *mut u8, msm_points: *mut u8) -> c_int;
    pub fn zkp_prove_phase_a(st: *const zkp_statement, n: u32, transcripts: *mut u8, secrets: *const u8, inst_points: *const u8,
                             common_points: *const u8, entropy: *const u8, n_threads: c_int, blindings: *mut u8, off: *mut u32,
                             scalars: *mut u8, pidx: *mut u32) -> c_int;
    pub fn zkp_prove_phase_b(st: *const zkp_statement, n: u32, transcripts: *mut u8, secrets: *const u8, blindings: *const u8,
                             commitments: *const u8, n_threads: c_int, challenges: *mut u8, responses: *mut u8) -> c_int;
}

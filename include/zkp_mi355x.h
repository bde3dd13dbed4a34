/* zkp_mi355x.h -- C ABI of the MI355X (gfx950) ristretto255 MSM / codec engine.
 *
 * This is the drop-in boundary for the hot path of dalek-cryptography/zkp.
 * The reference has no FFI: the path sits behind three curve25519-dalek trait methods plus the
 * point codec.  Each entry point below names the reference call site(s) it replaces; the Rust
 * `-sys` binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   scalar  : 32 bytes, little-endian integer.  The MSM entry points (1), (2), (2b) accept any 256-bit value and use
 *             it as an integer multiplier (so non-canonical scalars give the same group element dalek's
 *             `Scalar` would after reduction mod l).  The fused VERIFY flows (2c) take proofs, and there the
 *             reference's rule applies: a response >= l (which serde would refuse to deserialise into a
 *             `Scalar`, proofs.rs:14-32) is a verification failure for that proof / batch, and a compact proof's
 *             challenge is compared byte for byte with the recomputed canonical one (verifier.rs:115).
 *   point   : 32 bytes, ristretto255 encoding (RFC 9496).  Decoding rejects exactly what
 *             `CompressedRistretto::decompress` rejects (non-canonical, negative s, non-square,
 *             negative t, y == 0).
 *   buffers : caller owned, not retained after return.  `_dev` variants take DEVICE pointers
 *             (hipMalloc / torch CUDA tensors), enqueue on the context's stream and do not
 *             synchronise; plain variants take HOST pointers, copy in/out and synchronise.
 *   return  : 0 = computed.  < 0 = infrastructure failure (see ZKP_ERR_*): NO output may be
 *             trusted, callers must fail closed (reference analogue: ProofError::VerificationFailure,
 *             src/errors.rs:6).  There is no CPU fallback inside this library.
 *   threads : one context per host thread / per GPU; a context is not re-entrant.
 */
#ifndef ZKP_MI355X_H
#define ZKP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_OK 0
#define ZKP_ERR_HIP (-1)        /* a HIP runtime call failed (zkp_last_error has the text)        */
#define ZKP_ERR_ARG (-2)        /* NULL pointer / inconsistent sizes / index out of range         */
#define ZKP_ERR_NO_DEVICE (-3)  /* no gfx950 device visible                                       */
#define ZKP_ERR_OOM (-4)        /* device allocation failed                                       */

/* flags for zkp_msm_many */
#define ZKP_VARTIME 0  /* replaces RistrettoPoint::vartime_multiscalar_mul (verifier.rs:97)        */
#define ZKP_CT 1       /* replaces RistrettoPoint::multiscalar_mul (prover.rs:94): the instruction */
                       /* stream and every address are independent of the scalars                  */

typedef struct zkp_ctx zkp_ctx;

/* One context per GPU (one process per GPU in multi-GPU jobs).  device_id is the HIP ordinal. */
int zkp_ctx_create(zkp_ctx** out, int device_id);
void zkp_ctx_destroy(zkp_ctx* ctx);
/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the
 * context's own stream. */
int zkp_ctx_set_stream(zkp_ctx* ctx, void* hip_stream);
int zkp_ctx_synchronize(zkp_ctx* ctx);
/* Text of the last error on this thread (never NULL). */
const char* zkp_last_error(void);
/* Library / build identification, e.g. "zkp-mi355x 0.1 gfx950". */
const char* zkp_version(void);

/* Tuning knobs (results never depend on them).
 *   ZKP_OPT_BATCH_ENCODE_MIN: calls of zkp_msm_many / the fused flows with at least this many outputs encode them as
 *     2 * H with H = sum (s_i / 2) P_i, which needs one field inversion per 65,536 outputs instead of an inverse square
 *     root per output (the identity behind curve25519-dalek's double_and_compress_batch): 10 x fewer instructions in the
 *     encoding step, three short kernels instead of one (default 65536: below that the extra latency outweighs the
 *     instructions saved; 0 = always, UINT64_MAX = never).  Unless the option is set, the asynchronous _dev
 *     entry points, whose callers keep many calls in flight, use 2048.
 *   ZKP_OPT_COMB_TEETH: comb-table shape zkp_msm_many_dev uses for points that two or more terms of a call multiply
 *     (4 or 16; default 4).  16 suits calls whose shared points carry about six or more terms each (16 instead of 64
 *     doublings per term, a 4 x larger table per point).  Every other entry point derives the shape from its inputs.
 *   ZKP_OPT_CT_SINGLE_USE_TABLES: how ZKP_CT calls serve a point that a single term multiplies.  1 = a comb table like the shared
 *     points (the 256 doublings run next to the other tables' chains: shortest call), 0 = a constant-time radix-16 ladder over
 *     the point's own eight multiples (26 % fewer instructions for that term, but a 321-operation dependent chain inside the
 *     term kernel), UINT64_MAX = default: the ladder in asynchronous _dev calls of 250,000 terms or more (a call that fills the
 *     chip on its own), tables otherwise.
 *   ZKP_OPT_DEV_OVERLAP: 1 = zkp_fused_prove_dev / _verify_compact_dev / _verify_batchable_dev run the half of their work that does not depend on the
 *     transcripts (decoding, classification, comb tables) on a second stream of the context, as the synchronous entry points
 *     always do: a shorter call, more cross-stream dependencies.  Default 0.  (Measured again in round 4 on a LONE call chain: 2.87 -> 3.17 ms per
 *     prove call of 20,480 proofs -- no gain there either.)  In a process that owns one hardware queue (GPU_MAX_HW_QUEUES=1) a capture records the
 *     flow without the fork: ROCm 7.2.0 crashes in hipGraphLaunch on a forked graph under that setting.
 *     2 (round 6) = the whole LATENCY SCHEDULE of the synchronous entry points on device buffers, for a caller that keeps ONE call in flight: the second
 *     stream as above -- for zkp_fused_batch_verify[_many]_dev too: the decompressions of the batch MSM (batch_verifier.rs:226) run next to the transcript
 *     chain --, comb tables built by four lanes per point, tables for single-use points, and transcript-chain wavefronts that own their SIMD
 *     (k_transcript_chain<true>).  One batch of 4096 CMZ proofs proven and batch-verified per call: 2.53 M proofs/s against 2.30 M on the default schedule
 *     and 2.05 M in round 5 (bench.py: lone_call).
 *   ZKP_OPT_GROUPED_COMB: 1 = constant-time calls list the terms of every point with 10 or more uses next to each other; a wavefront
 *     then holds the rows of the (at most 8) 16-teeth comb tables its 62 terms need and every lane takes the entry its digit names over
 *     the lane crossbar (ZKP_OPT_CT_LOOKUP: no masked scan, 20 % fewer instructions per addition, a row fetched once per wavefront instead
 *     of once per lane); 0 = every comb term scans its rows with masks; UINT64_MAX = default: 1 for calls of 400,000 terms or more
 *     (asynchronous _dev calls: 250,000).
 *   ZKP_OPT_TABLES_LANE: comb tables are built by one lane per point (1: half the instructions) or by four lanes per point
 *     (0: a quarter of the latency); UINT64_MAX = default: 1 in the asynchronous _dev entry points, 0 in the synchronous ones.
 *   ZKP_OPT_FUSE_TABLES_TRANSCRIPT: 1 = zkp_fused_prove_dev / _verify_compact_dev run their first transcript program in the same
 *     launch as the comb-table construction (both are long dependent chains on few wavefronts, independent of each other): a
 *     lone call of 4096 CMZ proofs takes 1.37 instead of 1.92 ms (one such call after the other, prove + batch verify: 1.36 -> 1.68 M
 *     proofs/s; four call chains in flight: 3.27 -> 3.70 M), while callers that keep 25 such calls in flight lose 9 % (the transcript
 *     wavefronts then carry the table builder's 212 registers instead of their own 118) -- they are better served by one wide call
 *     (zkp_fused_prove_dev over K * 4096 proofs + zkp_fused_batch_verify_many_dev: 6.1 - 6.9 M proofs/s).  0 = never; UINT64_MAX =
 *     default: in calls of fewer than 65,536 proofs (from there on separate launches are 1.5 - 3 % faster).
 *   ZKP_OPT_TRANSCRIPT_LANES: lanes per proof in the Merlin transcript kernel of the fused flows.  2 = a lane pair per proof
 *     (each lane holds one 32-bit half of every STROBE word: half the latency), 1 = one lane per proof (23 % fewer
 *     instructions per Keccak-f), UINT64_MAX = default: 1 in asynchronous _dev calls of 65,536 proofs or more, 2 otherwise.
 *   ZKP_OPT_CT_LOOKUP: how a ZKP_CT call picks the table entry a secret digit names.
 *     0 / UINT64_MAX (default since round 5) = LANE CROSSBAR: constant time by construction.  A wavefront holds the row in registers, one
 *       entry per lane (fixed-base rows: 32 entries of a 6-bit window; grouped comb rows: 8 tables x 8 entries), and every lane fetches its
 *       entry with ds_bpermute_b32 -- the digit selects a source LANE, never a memory address, and the layouts keep the sources of every
 *       instruction inside one 32-lane half, where the crossbar has no bank conflicts whatever the digits are (hot_tables.h, comb_tables.h;
 *       tools/microbench/bpermute_rate.hip).  Rows of 8 entries that belong to ONE lane (comb tables of points with fewer than 11 uses,
 *       ladder tables) are scanned completely and the entry kept with v_cndmask, as curve25519-dalek's LookupTable::select does.  This is
 *       what `RistrettoPoint::multiscalar_mul` promises at prover.rs:94, at the speed of the look-up of value 2 (profiles/r05_ab_experiments.txt).
 *     1 = MASKED SCANS everywhere (fixed-base rows: 32 entries x 7 LDS reads + 864 selects per addition; no grouped comb walk): the
 *       round-3 "safe mode"; same bytes, -25 % throughput.  Kept as the reference point of the other two.
 *     2 = the default of rounds 2 - 4: rows replicated in LDS and read at an index derived from the digit, from banks that no other lane of
 *       the ds_read_b128 service group touches -- constant time under the LDS bank / service-group model of the hardware guide (checked
 *       with PMC counters and per-wavefront cycle counts), not by construction.
 *     Same bytes out for every value (tests/test_gpu_device_entry.py); 1 and 2 exist for the 6-bit fixed-base window only.
 *   ZKP_OPT_CT_MASKED_SCANS: the name ZKP_OPT_CT_LOOKUP had in rounds 3 - 4 (same id; value 1 still selects the masked scans, value 0 is now the crossbar).
 *   ZKP_OPT_EACH_STRAUS: how zkp_fused_verify_batchable[_dev] computes a proof's MSM over its points and commitments (verifier.rs:162-166).
 *     UINT64_MAX = default: one Straus walk per proof -- 256 shared doublings and one table addition per operand and window; below
 *     65,536 proofs split over 32 lanes per proof by windows (each lane: two windows of every operand; one quad of lanes per proof then
 *     joins the partial sums), from 65,536 proofs on one lane per proof.  0x200 + P (P = 1, 2, 4 .. 64) = P window parts per proof;
 *     1 .. 8 = split by operands over that many lanes per proof (every lane runs the 256 doublings); 0 = the round-2 schedule
 *     (every single-use point on a ladder of its own: 256 doublings per operand).
 *   ZKP_OPT_LADDER_INTERLEAVE: 1 = the term kernel's ladder blocks (single-use points: CMZ's Q) are spread over the first half of its grid
 *     instead of all starting first (fewer per-lane ladder tables in flight together: -20 % HBM fetch in that kernel); 0 = all first;
 *     UINT64_MAX = default: spread when the launch has 256 or more ladder blocks (65,536 single-use points), where it also is ~1 % faster --
 *     in a lone smaller launch the later start of the last ladder block lengthens the kernel (profiles/r03_ab_experiments.txt, block l).
 *   ZKP_OPT_JOB_DEFER_D2H: when the device -> host copies of a host-buffer job (section 2d) are issued.  1 (default) = by zkp_ctx_job_poll /
 *     zkp_ctx_job_wait once the job's kernels are finished; 0 = queued behind the kernels at submit.  The copy engines serve ONE queue in order:
 *     a copy that waits in it for its job's kernels (milliseconds) holds up the copies IN of every job submitted after it -- measured with six
 *     contexts, a job's inputs take 3.7 ms to arrive instead of 1.4, and the pipelined rate through pinned buffers is 4.5 instead of 5.4 M proofs/s
 *     (profiles/r04_ab_experiments.txt, block e).
 *   ZKP_OPT_SYNC_SCHEDULE: which schedule the SYNCHRONOUS host-pointer entry points (section 2c) run.  0 / UINT64_MAX (default) = the low-latency one (second
 *     stream for the point phase, comb tables built by four lanes per point, single-use points on tables): one call at a time per process, the caller sees
 *     the call's duration.  1 = the throughput schedule of the asynchronous jobs (section 2d): for callers that issue synchronous calls from several host
 *     threads at once, one context per thread -- every call is a little longer, the chip does less work per proof (profiles/r04_ab_experiments.txt, block r).
 *   ZKP_OPT_WS_LIMIT_BYTES: the largest device workspace this context may allocate (it grows with the largest call it has served: ~85 KB per CMZ
 *     proof of a prove call, 9 KB of it the transcript images).  A call that would need more returns ZKP_ERR_OOM instead of allocating -- the way to keep several contexts of a
 *     zkp_pipe (zkp_toolbox.h) inside one GPU's memory.  0 / UINT64_MAX = no cap (default).
 *   ZKP_OPT_TRANSCRIPT_STEPS: how the lane-pair Merlin transcripts of the fused flows run (round 6).  1 (default) = assemble + chain: one wide kernel builds every
 *     proof's per-block absorb image (all loads independent; identity checks too), then a chain kernel does nothing but state = (state & KEEP) ^ image and
 *     Keccak-f[1600] per block, state in registers, the next image prefetched under the permutation -- 5.6 us per permutation on a lone wavefront instead of the
 *     9 - 14 us of the word-operation interpreter, whose every operation is a dependent global load (profiles/r06_keccak_microbench.txt, r06_ab_experiments.txt).
 *     0 = the interpreter of rounds 2 - 5 (same bytes).  Calls wide enough for one transcript lane per proof (ZKP_OPT_TRANSCRIPT_LANES) keep the interpreter.
 *   ZKP_OPT_COMB_SPLIT: constant-time calls, the terms of a per-call point with 2 - 9 uses (or one use and a table: CMZ's Q) scan their 8-entry rows completely; one
 *     lane per term is a chain of 64 scanned additions.  1 = a QUAD of lanes per such term, one window each (16 scanned additions per lane, then a 12-doubling
 *     Horner inside the quad: a third of the chain for 1.45 x the instructions), together with the grouped walk for the points that qualify.  Default
 *     (UINT64_MAX): calls of 8,192 .. 400,000 terms on the latency schedule (synchronous entry points, ZKP_OPT_DEV_OVERLAP = 2); 0 = never.  Same bytes.
 *   ZKP_OPT_JOINT_LADDER: variable-time statement flows (zkp_fused_verify_compact*: commitment = sum s_i P_i - c LHS per constraint, verifier.rs:95-106).  The
 *     left-hand side is multiplied once per proof -- a chain of 252 doublings of its own.  1 (default): that chain also carries ONE other per-proof term of the
 *     constraint (Straus interleaving: eight multiples + 64 additions, no doublings, no comb table) -- CMZ: P joins C_i's chain in ten constraints and needs no
 *     table, Q joins V's: 11 chains instead of 12 and no 16-teeth table per proof.  A per-proof point ALL of whose terms ride (P) gets a table of its multiples
 *     1 .. 128 where its comb table was: its riders add one signed 8-bit digit per byte (32 additions instead of 64) and build no multiples of their own;
 *     (a table is a chain of 127 additions: built on the throughput schedule and in calls of >= 16,384 proofs, not in a lone synchronous call of fewer);
 *     2 = pairs without these tables.  0 = every term on its own (rounds 2 - 5).  Same bytes.
 *   This enum is the whole option surface of the shipped library; measurement hooks live in test-hook builds only (end of file). */
enum { ZKP_OPT_BATCH_ENCODE_MIN = 1, ZKP_OPT_COMB_TEETH = 2, ZKP_OPT_CT_SINGLE_USE_TABLES = 3, ZKP_OPT_TRANSCRIPT_LANES = 4, ZKP_OPT_DEV_OVERLAP = 5, ZKP_OPT_GROUPED_COMB = 6, ZKP_OPT_TABLES_LANE = 7,
       ZKP_OPT_FUSE_TABLES_TRANSCRIPT = 8, ZKP_OPT_CT_LOOKUP = 9, ZKP_OPT_CT_MASKED_SCANS = 9 /* round-3 name: value 1 still selects the scans */, ZKP_OPT_EACH_STRAUS = 10, ZKP_OPT_LADDER_INTERLEAVE = 11, ZKP_OPT_WS_LIMIT_BYTES = 12, ZKP_OPT_JOB_DEFER_D2H = 13, ZKP_OPT_SYNC_SCHEDULE = 14, ZKP_OPT_TRANSCRIPT_STEPS = 15, ZKP_OPT_COMB_SPLIT = 16, ZKP_OPT_JOINT_LADDER = 17 };
int zkp_ctx_set_option(zkp_ctx* ctx, int option, uint64_t value);

/* HIP graphs.  A batch of proofs is a chain of ~35 short kernels (75 in round 1); enqueueing them one by one costs the host ~0.1 ms per
 * batch (measured: 0.14-0.17 ms against 0.9 ms of GPU time per pipelined batch; 0.025 ms as a graph), which matters for
 * short runs and for hosts busier than a benchmark loop.  Everything enqueued on the context's stream between _begin and
 * _end -- *_dev calls of this library and
 * the caller's own asynchronous copies on that stream -- is recorded instead of executed; zkp_graph_launch then replays
 * the recording with ONE host call.  Replays read and write the same device addresses, so the buffers must stay alive
 * and are reused by every replay.  Preconditions: the same calls ran once before on this context with the same shapes
 * (statement plans compiled, workspace sized, fixed points registered) -- otherwise ZKP_ERR_ARG -- and profiling is off.
 * Lifetime rules.  A graph belongs to the context it was captured on: the recorded kernels hold raw addresses inside that
 * context's workspace and statement plans.  Each graph is stamped with the context's workspace / plan generation;
 * zkp_graph_launch returns ZKP_ERR_ARG ("stale graph") -- it never runs the recording -- when, after the capture, a larger
 * call made the workspace grow (it is reallocated), the plan cache was flushed (more than 64 distinct (flow, statement, N)
 * plans on one context), the context was destroyed, or when the graph is offered to another context.  Capture again then.
 * If a call between _begin and _end fails, the capture is poisoned: call zkp_ctx_capture_abort (ends and discards it; the
 * context is usable again) -- zkp_ctx_capture_end on a poisoned capture returns an error and also leaves capture mode. */
typedef struct zkp_graph zkp_graph;
int zkp_ctx_capture_begin(zkp_ctx* ctx);
int zkp_ctx_capture_end(zkp_ctx* ctx, zkp_graph** out);
int zkp_ctx_capture_abort(zkp_ctx* ctx);                /* no capture in progress: no-op */
int zkp_graph_launch(zkp_graph* graph, zkp_ctx* ctx);   /* asynchronous, on the context's current stream */
void zkp_graph_destroy(zkp_graph* graph);

/* Performance hint, never changes a result: declare points that very many terms of later zkp_msm_many calls
 * will reference -- in the reference's vocabulary the statement's COMMON variables (define_proof!,
 * macros.rs:84,236-242) / BatchVerifier's static points (batch_verifier.rs:100-112), e.g. the issuer
 * parameters X_1..X_10, A of the CMZ'13 statement.  The engine builds fixed-base window tables for them once
 * (64 slots, least-recently-used replacement) and then serves every term on such a point with 43 mixed
 * additions and no doublings (154 KB of table per point).  encodings = HOST pointer [n][32]; synchronous. */
int zkp_ctx_prepare_fixed_points(zkp_ctx* ctx, uint32_t n, const uint8_t* encodings);

/* (1) Many small multiscalar multiplications in CSR form, fused with compression.
 *     Replaces, for a whole batch of proofs at once:
 *       prover.rs:94-97   RistrettoPoint::multiscalar_mul(..)            (flags = ZKP_CT)
 *       verifier.rs:97-106 RistrettoPoint::vartime_multiscalar_mul(..)   (flags = ZKP_VARTIME)
 *     and the `point.compress()` of toolbox/mod.rs:204 applied to each result.
 *       out[i]    = encode( sum_{t in [off[i], off[i+1])} scalars[t] * decode(points[pidx[t]]) )
 *       status[i] = 0 ok | 1 some referenced point failed to decode (Rust: decompress() == None;
 *                   out[i] is then 32 zero bytes and must not be used)
 *     off has n_msm+1 entries, off[0] = 0, non-decreasing; T = off[n_msm] terms. An empty range
 *     yields the identity encoding (32 zero bytes), like an empty dalek MSM. */
int zkp_msm_many(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off, const uint8_t* scalars /*[T][32]*/,
                 const uint32_t* pidx /*[T]*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points,
                 int flags, uint8_t* out /*[n_msm][32]*/, uint8_t* status /*[n_msm]*/);
int zkp_msm_many_dev(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* d_off, const uint8_t* d_scalars,
                     const uint32_t* d_pidx, const uint8_t* d_points, uint32_t n_points, uint32_t n_terms,
                     int flags, uint8_t* d_out, uint8_t* d_status);

/* (2) One large multiscalar multiplication with decode-or-None.
 *     Replaces RistrettoPoint::optional_multiscalar_mul(scalars, points.map(decompress)) at
 *       verifier.rs:162-166 and batch_verifier.rs:219-228 (the batch-verification random linear
 *       combination of size num_s + (num_i + num_c) * N).
 *     *status = 0: Some(P), out_point = encode(P) (callers test for 32 zero bytes = identity,
 *                  verifier.rs:168 / batch_verifier.rs:230)
 *             = 1: None (some point failed to decode); out_point is zeroed and meaningless. */
int zkp_msm_optional(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars /*[n][32]*/,
                     const uint8_t* points /*[n][32]*/, uint8_t out_point[32], int* status);
int zkp_msm_optional_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_scalars, const uint8_t* d_points,
                         uint8_t* d_out_point /*[32]*/, uint32_t* d_status /*[1]*/);

/* (2b) Batch verification with the coefficient build ON THE GPU.
 *     Replaces batch_verifier.rs:173-234 in one call: the random-linear-combination coefficients
 *       static_coeffs[s]        = sum_j sum_{constraint i touching s} r_ij * (minus_c_j | resp_j[sc])      (:185-204)
 *       Matrix[(var, j)]        likewise for instance variables, and  Matrix[(n_i + i, j)] = -r_ij        (:183)
 *     are computed with on-device arithmetic mod l, laid out as the reference chains them (:219-223: static
 *     coefficients, then the matrix row-major), and fed to the same MSM as zkp_msm_optional together with
 *     static_points || instance_points || commitment rows.  Point ids: 0 .. n_static-1 = static points,
 *     n_static .. n_static+n_instance-1 = instance points.  All pointers are HOST pointers.
 *     minus_c [N][32] = the negated per-proof challenges (:163-167, computed by the caller's transcripts);
 *     responses [N][n_secrets][32]; weights16 [n_constraints][N][16] = the u128 random factors (:179), little endian;
 *     instance_points [n_instance][N][32]; commitments [N][n_constraints][32].
 *     *status as in zkp_msm_optional.  debug_scalars (NULL or [n_static + (n_instance+n_constraints)*N][32]) receives
 *     the coefficient vector for tests. */
typedef struct {
  uint32_t n_secrets, n_static, n_instance, n_constraints;
  const uint32_t* cons_lhs;   /* [n_constraints] point id of the left-hand side          */
  const uint32_t* cons_off;   /* [n_constraints + 1] offsets into cons_sc / cons_pt      */
  const uint32_t* cons_sc;    /* secret index of each right-hand-side term               */
  const uint32_t* cons_pt;    /* point id of each right-hand-side term                   */
} zkp_batch_statement;
int zkp_batch_check(zkp_ctx* ctx, const zkp_batch_statement* st, uint32_t N, const uint8_t* minus_c,
                    const uint8_t* responses, const uint8_t* weights16, const uint8_t* static_points,
                    const uint8_t* instance_points, const uint8_t* commitments, uint8_t out_point[32], int* status,
                    uint8_t* debug_scalars);

/* (2c) Fused statement flows: a whole batch of proofs of ONE statement handled
 *     on the device -- Merlin/STROBE transcripts (src/toolbox/mod.rs:165-228 over merlin 2.x), blinding factors
 *     (prover.rs:78-89), scalar arithmetic mod l (prover.rs:107-109, batch_verifier.rs:173-206), MSM operand assembly
 *     and the MSMs themselves.  The host uploads inputs and downloads proofs or verdicts; nothing else crosses PCIe.
 *     `transcripts` = [N][208] transcript blobs (layout of zkp_toolbox.h: 200 bytes of STROBE state, then pos,
 *     pos_begin, cur_flags), updated in place exactly as the reference updates its `&mut Transcript`s.  All N blobs
 *     must stand at the same STROBE position (same pos / pos_begin / cur_flags bytes), which holds whenever they were
 *     produced by the same sequence of appends with equal lengths; otherwise ZKP_ERR_ARG (callers then use the
 *     per-proof host transcripts of zkp_toolbox.h).  Layouts: secrets / responses [N][n_secrets][32];
 *     inst [n_instance][N][32]; common [n_static][32]; commitments [N][n_constraints][32]; entropy [N][32] (the 32
 *     bytes the external RNG contributes to each proof's TranscriptRng, prover.rs:82).
 *     Witnesses need not be reduced: `secrets` holds each Scalar's 32 bytes as the caller allocated it, and any 256-bit value is
 *     accepted (a Rust binding passes Scalar::as_bytes(), also of a Scalar::from_bits value).  As in the reference, the prover's RNG
 *     is re-keyed with those 32 bytes AS GIVEN (prover.rs:80), so s and s + l draw different blindings and give different -- both
 *     valid -- proofs; the response is (s mod l) * c + b mod l (prover.rs:107-109).  Every output (challenges, responses,
 *     commitments) is canonical whatever the witness bytes were.  The same holds for d_secrets of the _dev entry points.
 *     (tests/degenerate_cases.py: non-canonical witnesses on every route against both oracles, byte for byte.) */
typedef struct {
  zkp_batch_statement shape;
  const char* label;                  /* the proof label of `domain_sep` (mod.rs:166-169)                                  */
  const char* const* secret_labels;   /* [n_secrets]                                                                      */
  const char* const* point_labels;    /* [n_static + n_instance], indexed by point id                                     */
  const uint32_t* alloc_order;        /* [n_static + n_instance] point ids in allocation (= transcript) order             */
  const uint32_t* alloc_seq;          /* NULL: every secret is allocated before the first point (define_proof!'s order,   */
                                      /* macros.rs:215-242).  Otherwise [n_secrets + n_static + n_instance] entries, the  */
                                      /* caller's allocate_scalar / allocate_point calls in order: 0x80000000 | secret     */
                                      /* index, or a point id (the points must come in alloc_order's order).              */
} zkp_fused_statement;
/* N x { build_prover (macros.rs:206-258) ; Prover::prove_impl (prover.rs:76-112) }.  *invalid_point = 1 if some input
 * encoding did not decode (the reference prover holds decoded points, so this is a caller bug there). */
int zkp_fused_prove(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                    const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, uint8_t* challenges,
                    uint8_t* responses, uint8_t* commitments, int* invalid_point);
/* The same with the prover's entropy drawn ON THE DEVICE (round 6): seed = 40 bytes the caller took from the operating system; proof j's 32 bytes of
 * `thread_rng()` (prover.rs:82) are bytes [32 j, 32 j + 32) of the ChaCha20 stream keyed with seed[0..32), nonce seed[32..40) -- what the asynchronous jobs of
 * section 2d do.  Drawing 32 N bytes on the host costs a synchronous call of 4096 proofs ~0.1 ms, the batch verifier's 16 N n_constraints bytes ~0.2 ms. */
int zkp_fused_prove_seeded(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                           const uint8_t* inst, const uint8_t* common, const uint8_t seed[40], uint8_t* challenges,
                           uint8_t* responses, uint8_t* commitments, int* invalid_point);
/* N x { build_verifier (macros.rs:280-311) ; Verifier::verify_compact (verifier.rs:80-120) }.  results[j]: 0 = accepted. */
int zkp_fused_verify_compact(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                             const uint8_t* inst, const uint8_t* common, const uint8_t* challenges,
                             const uint8_t* responses, uint8_t* results);
/* batch_verify (macros.rs:336-370 ; batch_verifier.rs:67-235) without the batch-shape checks, which stay with the
 * caller.  weights16 [n_constraints][N][16].  *verdict: 0 = the batch verifies.  debug_scalars as in zkp_batch_check. */
int zkp_fused_batch_verify(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                           const uint8_t* inst, const uint8_t* common, const uint8_t* commitments,
                           const uint8_t* responses, const uint8_t* weights16, int* verdict, uint8_t* debug_scalars);

/* K independent batch verifications in ONE pass (K x batch_verifier.rs:67-235), for servers that collect more proofs than
 * they want to tie to one verdict: the K * N_each proofs lie next to each other in every array, batch b = proofs
 * [b * N_each, (b + 1) * N_each).  Each batch gets what BatchVerifier::verify_batchable gives it: its own weights, its own
 * sums of the static-point coefficients (:187, :198), its own MSM of n_static + (n_instance + n_constraints) * N_each terms
 * (:219-228) and its own verdict -- a bad proof, a rejected point or an undecodable point in batch b changes verdict b only.
 * One transcript launch, one coefficient grid and one "segmented" Pippenger (sort key = (batch, window, digit)) serve all K
 * batches, so the narrow tails of a single batch check (bucket tree, Horner) are K times wider.
 * Layouts as in zkp_fused_batch_verify with N = K * N_each: transcripts [N][208], inst [n_instance][N][32], commitments
 * [N][n_constraints][32], responses [N][n_secrets][32], weights16 [n_constraints][N][16].  verdicts [K]: 0 = batch b verifies.
 * debug_scalars (NULL or [K * n_static + (n_instance + n_constraints) * N][32]): static coefficients batch by batch, then the
 * coefficient matrix row-major over all N proofs.  K = 1 is zkp_fused_batch_verify. */
int zkp_fused_batch_verify_many(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t n_batches, uint32_t N_each, uint8_t* transcripts,
                                const uint8_t* inst, const uint8_t* common, const uint8_t* commitments, const uint8_t* responses,
                                const uint8_t* weights16, int* verdicts, uint8_t* debug_scalars);
/* The same with the weights of batch_verifier.rs:179 drawn on the device from the ChaCha20 stream of a 40-byte seed (see zkp_fused_prove_seeded): weight
 * (constraint k, proof j) = bytes [16 (k N + j), + 16) of the stream. */
int zkp_fused_batch_verify_many_seeded(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t n_batches, uint32_t N_each, uint8_t* transcripts,
                                       const uint8_t* inst, const uint8_t* common, const uint8_t* commitments, const uint8_t* responses,
                                       const uint8_t seed[40], int* verdicts);

/* N x { build_verifier ; Verifier::verify_batchable (verifier.rs:123-173) }: one MSM of (points + commitments) terms per
 * proof, folded with the 128-bit weights16 [N][n_constraints][16] (verifier.rs:153).  results[j]: 0 = accepted.  This is
 * the per-proof check that localises a bad proof after a failed batch verification. */
int zkp_fused_verify_batchable(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                               const uint8_t* inst, const uint8_t* common, const uint8_t* commitments,
                               const uint8_t* responses, const uint8_t* weights16, uint8_t* results);
/* The same, additionally returning the per-proof coefficient vectors the device folded (verifier.rs:144-160): debug_scalars
 * = NULL or [N][n_static + n_instance + n_constraints][32], per proof in the operand order of verifier.rs:162-166 (the
 * points by point id, then the commitments), so tests can compare them with a restatement of the fold. */
int zkp_fused_verify_batchable_coeffs(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                                      const uint8_t* inst, const uint8_t* common, const uint8_t* commitments,
                                      const uint8_t* responses, const uint8_t* weights16, uint8_t* results,
                                      uint8_t* debug_scalars);

/* Ragged batches: the calls above for transcripts at different STROBE positions (aligned batches are accepted too).  Synchronous, host
 * pointers, ZKP_ERR_ARG during graph capture.  Prove takes entropy [N][32] or a 40-byte seed, batch verification weights16 or a seed: exactly one. */
int zkp_fused_prove_ragged(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts, const uint8_t* secrets,
                           const uint8_t* inst, const uint8_t* common, const uint8_t* entropy, const uint8_t seed[40], uint8_t* challenges,
                           uint8_t* responses, uint8_t* commitments, int* invalid_point);
int zkp_fused_verify_compact_ragged(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                                    const uint8_t* inst, const uint8_t* common, const uint8_t* challenges,
                                    const uint8_t* responses, uint8_t* results);
int zkp_fused_verify_batchable_ragged(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint8_t* transcripts,
                                      const uint8_t* inst, const uint8_t* common, const uint8_t* commitments,
                                      const uint8_t* responses, const uint8_t* weights16, uint8_t* results);
int zkp_fused_batch_verify_many_ragged(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t n_batches, uint32_t N_each, uint8_t* transcripts,
                                       const uint8_t* inst, const uint8_t* common, const uint8_t* commitments, const uint8_t* responses,
                                       const uint8_t* weights16, const uint8_t seed[40], int* verdicts);

/*     Device-resident variants: every buffer is a device pointer (16-byte aligned), nothing is copied and the call
 *     returns as soon as the work is queued on the context's stream (zkp_ctx_synchronize to wait).  strobe_pos =
 *     pos | pos_begin << 8 | cur_flags << 16, the three trailing bytes every one of the N transcript blobs holds.
 *     d_table = common points followed by the instance rows: [n_static + n_instance * N][32].
 *     zkp_fused_prove_dev: d_status [N * n_constraints] bytes, non-zero where an input point failed to decode.
 *     zkp_fused_batch_verify_dev: d_points [n_static + (n_instance + n_constraints) * N][32] with the static points
 *     and instance rows filled in (the commitment rows are written by the call); d_status [2] words: decode failure
 *     in the MSM | a point or commitment rejected by the transcript protocol (identity encoding); the batch verifies
 *     iff both are 0 and d_out_point holds 32 zero bytes (= the canonical encoding of the identity; for any other sum the 32 bytes are a
 *     non-zero marker, not its encoding: batch_verifier.rs:230-234 asks is_identity() and nothing else, and the test -- X = 0 or Y = 0 --
 *     needs no inverse square root at the end of the MSM's 253-doubling chain). */
int zkp_fused_prove_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t strobe_pos, uint8_t* d_transcripts,
                        const uint8_t* d_secrets, const uint8_t* d_table, const uint8_t* d_entropy, uint8_t* d_challenges,
                        uint8_t* d_responses, uint8_t* d_commitments, uint8_t* d_status);
int zkp_fused_verify_compact_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t strobe_pos,
                                 uint8_t* d_transcripts, const uint8_t* d_table, const uint8_t* d_challenges,
                                 const uint8_t* d_responses, uint8_t* d_results);
int zkp_fused_batch_verify_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t strobe_pos,
                               uint8_t* d_transcripts, uint8_t* d_points, const uint8_t* d_commitments,
                               const uint8_t* d_responses, const uint8_t* d_weights16, uint8_t* d_out_point,
                               uint32_t* d_status);
/*     zkp_fused_verify_batchable_dev (verifier.rs:123-173 for N proofs, one verdict per proof): d_table = common points, instance rows and
 *     then the proofs' commitments, [n_static + n_instance * N][32] || [N][n_constraints][32]; d_weights16 [N][n_constraints][16] (the
 *     factors verifier.rs:153 draws per proof); d_results [N] bytes, 0 = verified. */
int zkp_fused_verify_batchable_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t strobe_pos,
                                   uint8_t* d_transcripts, const uint8_t* d_table, const uint8_t* d_responses,
                                   const uint8_t* d_weights16, uint8_t* d_results);

/* zkp_fused_batch_verify_many on device buffers: d_points [n_static + (n_instance + n_constraints) * N][32] (N = n_batches *
 * N_each; static points and instance rows filled in, commitment rows written by the call), d_out_points [n_batches][32],
 * d_status [n_batches][2] words (decode failure in batch b's MSM | a point, commitment or response of batch b rejected):
 * batch b verifies iff both are 0 and d_out_points[b] is 32 zero bytes (otherwise a non-zero marker, as above). */
int zkp_fused_batch_verify_many_dev(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t n_batches, uint32_t N_each, uint32_t strobe_pos,
                                    uint8_t* d_transcripts, uint8_t* d_points, const uint8_t* d_commitments, const uint8_t* d_responses,
                                    const uint8_t* d_weights16, uint8_t* d_out_points, uint32_t* d_status);

/* (2d) The fused flows on HOST buffers as asynchronous jobs (round 4).  One job per context at a time:
 *       zkp_fused_*_submit   queues host -> device copies, the flow and device -> host copies on the context's stream and returns;
 *       zkp_ctx_job_wait     blocks until that job is done and writes what needs the host (verdicts, invalid_point).
 *     The synchronous host-pointer calls of (2c) are exactly submit + wait.  A caller that wants throughput keeps SEVERAL contexts busy --
 *     on one GPU or on several (zkp_pipe of zkp_toolbox.h does that): the copies of one job overlap the kernels of the others.
 *     Host buffers: every input and output buffer named by a submit must stay valid and untouched until zkp_ctx_job_wait returns.  Pinned
 *     memory (zkp_host_alloc / zkp_host_register) makes the copies truly asynchronous; with ordinary memory HIP stages each copy and the
 *     submit call blocks for its duration (same results).
 *     flags: ZKP_JOB_SHARED_TRANSCRIPT -- `transcripts` is ONE 208-byte blob that every proof starts from (the reference's callers write
 *       `Transcript::new(label)` per proof: tests/zkp.rs:44, benches/zkp.rs:60) instead of [N][208].
 *     transcripts_out: NULL, or [N][208] receiving the advanced transcripts (what the reference leaves in its `&mut Transcript`s).
 *     inst_stride: proofs per row of the caller's `inst` array, >= N: row r of this job's instance points starts at inst + 32 * r * inst_stride.
 *       A job over the proof range [j0, j0 + N) of a larger batch passes inst + 32 * j0 and the batch size (weights_stride likewise for
 *       the [n_constraints][.][16] weights of the batch verifier) -- no gathering of columns on the host.
 *     entropy / weights16 == NULL: drawn ON THE DEVICE from the ChaCha20 stream (RFC 8439 block function, 64-bit counter from 0, 64-bit nonce)
 *       keyed with rng_seed[40] = key[32] || nonce[8], which the caller takes from the operating system per job -- what `thread_rng()` is
 *       to the reference (prover.rs:82, verifier.rs:153, batch_verifier.rs:179: rand 0.7's ThreadRng is a ChaCha stream keyed from the OS);
 *       entropy[j] = stream bytes [32 j, 32 j + 32), weights16 = the first 16 * n_constraints * N stream bytes in the array's own order.
 *     Errors (fail closed): the verdict words of a job -- results[N] of the two per-proof verifiers, verdicts[n_batches] of the batch verifier --
 *       are set to 1 (rejected) by the submit call itself as soon as its pointers have been checked, and only a job that ran to its end
 *       overwrites them: a failed submit (which leaves no job pending and has waited for whatever it had queued: the caller's buffers are free
 *       again) and a failed zkp_ctx_job_wait (< 0: the device failed underneath the job, or a copy out could not be issued by an earlier
 *       zkp_ctx_job_poll) both leave every verdict at "rejected", *invalid_point at 1, and no output buffer may be used.  The pinned words a
 *       wait derives verdicts from are poisoned at every submit, so nothing an earlier job left behind can read as "verified".
 *       Any other call on a context with a pending job returns ZKP_ERR_ARG.
 *     zkp_ctx_job_discard: for an owner that goes away with a job in flight (zkp_pipe_destroy): waits for the job's kernels, issues no copy
 *       out that was not already queued (with the default of ZKP_OPT_JOB_DEFER_D2H -- deferred copies --: none) and writes nothing to the caller's memory. */
#define ZKP_JOB_SHARED_TRANSCRIPT 1u
int zkp_fused_prove_submit(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                           const uint8_t* secrets, const uint8_t* inst, uint32_t inst_stride, const uint8_t* common,
                           const uint8_t* entropy, const uint8_t* rng_seed /*[40], used when entropy == NULL*/, uint8_t* transcripts_out,
                           uint8_t* challenges, uint8_t* responses, uint8_t* commitments, int* invalid_point);
int zkp_fused_verify_compact_submit(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                                    const uint8_t* inst, uint32_t inst_stride, const uint8_t* common, const uint8_t* challenges,
                                    const uint8_t* responses, uint8_t* transcripts_out, uint8_t* results /*[N]*/);
int zkp_fused_batch_verify_many_submit(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t n_batches, uint32_t N_each, uint32_t flags,
                                       const uint8_t* transcripts, const uint8_t* inst, uint32_t inst_stride, const uint8_t* common,
                                       const uint8_t* commitments, const uint8_t* responses, const uint8_t* weights16,
                                       uint32_t weights_stride, const uint8_t* rng_seed, uint8_t* transcripts_out, int* verdicts /*[n_batches]*/);
int zkp_fused_verify_batchable_submit(zkp_ctx* ctx, const zkp_fused_statement* st, uint32_t N, uint32_t flags, const uint8_t* transcripts,
                                      const uint8_t* inst, uint32_t inst_stride, const uint8_t* common, const uint8_t* commitments,
                                      const uint8_t* responses, const uint8_t* weights16 /*[N][n_constraints][16]*/, const uint8_t* rng_seed,
                                      uint8_t* transcripts_out, uint8_t* results /*[N]*/);
int zkp_ctx_job_wait(zkp_ctx* ctx);      /* no job pending: ZKP_OK at once */
int zkp_ctx_job_poll(zkp_ctx* ctx);      /* 1 = zkp_ctx_job_wait would not block, 0 = still running.  Polling also moves the job along: its copies
                                          * out are issued by the first poll (or wait) that finds its kernels finished -- see ZKP_OPT_JOB_DEFER_D2H */
int zkp_ctx_job_pending(zkp_ctx* ctx);   /* 1 = a job was submitted and not yet waited for */
int zkp_ctx_job_discard(zkp_ctx* ctx);   /* forget the pending job without touching the caller's memory (see Errors above) */
/* With zkp_ctx_set_profiling(ctx, 1): where the last finished job spent its time ON ITS STREAM, from HIP events recorded on that stream --
 * ms[0] host -> device copies (+ on-device randomness), ms[1] the flow's kernels, ms[2] device -> host copies.  Under load these include the
 * time the stream waited for the chip / the copy engines, which is what a pipelining caller wants to see. */
int zkp_ctx_job_timing(zkp_ctx* ctx, float ms[3]);

/* Pinned host memory for the jobs above (hipHostMalloc / hipHostRegister, visible to every GPU of the process).  zkp_host_is_pinned: 1 if p
 * points into such memory.  Registering costs ~12 us per MiB (profiles/r04_pcie_copy_rates.txt): register long-lived buffers once. */
int zkp_host_alloc(void** out, size_t bytes);
/* The same on the NUMA node of GPU `device` (round 5): on a two-socket host a staging buffer on the far socket sends every copied byte over the
 * socket interconnect first.  The runtime places pinned memory next to the calling thread's CURRENT device; zkp_host_alloc_on makes `device` current
 * for the allocation and restores the thread's device.  zkp_host_numa_node: the node the device hangs off (hipDeviceAttributeHostNumaId, else sysfs),
 * -1 = unknown; zkp_host_node_of: the node the page at p lives on (get_mempolicy), -1 = unknown / not permitted.  zkp_pipe's staging rings are
 * allocated this way (zkp_toolbox.h). */
int zkp_host_alloc_on(void** out, size_t bytes, int device);
int zkp_host_numa_node(int device);
int zkp_host_node_of(const void* p);
void zkp_host_free(void* p);
int zkp_host_register(void* p, size_t bytes);
int zkp_host_unregister(void* p);
int zkp_host_is_pinned(const void* p);

/* The device-side generator behind `entropy == NULL` / `weights16 == NULL`, exposed for the known-answer test: bytes (a multiple of 64)
 * of the ChaCha20 stream, block b = zkp_chacha20_block(key, first_block + b, nonce) of zkp_toolbox.h, into d_out (device, 16-byte aligned);
 * asynchronous on the context's stream. */
int zkp_chacha20_fill_dev(zkp_ctx* ctx, const uint8_t key[32], uint64_t nonce, uint64_t first_block, uint8_t* d_out, size_t bytes);

/* (3) Stand-alone decode / validity check, batched.  Replaces the
 *     `.map(|pt| pt.decompress()).collect::<Option<Vec<_>>>()` of verifier.rs:87-92.
 *     status[i] = 0 valid | 1 decompress() would return None.  If xyzt != NULL it receives the
 *     affine extended coordinates (X, Y, Z = 1, T) as 4 x 32-byte little-endian field elements. */
int zkp_decode_check(zkp_ctx* ctx, uint64_t n, const uint8_t* points /*[n][32]*/, uint8_t* status /*[n]*/,
                     uint8_t* xyzt /*[n][128] or NULL*/);

/* (4) Stand-alone encode.  Replaces `point.compress()` of mod.rs:180 for provers that hold
 *     uncompressed points (prover.rs:64-73).  Input: extended coordinates (X, Y, Z, T), each a
 *     32-byte little-endian field element (need not be reduced below p, bit 255 ignored). */
int zkp_encode_many(zkp_ctx* ctx, uint64_t n, const uint8_t* xyzt /*[n][128]*/, uint8_t* out /*[n][32]*/);

/* (5) Hash to the group, batched: RFC 9496 section 4.3.4 FROM_UNIFORM_BYTES, which is curve25519-dalek's
 *     `RistrettoPoint::from_uniform_bytes` (and, behind SHA-512 on the host, `hash_from_bytes::<Sha512>`).  out[i] = the
 *     canonical encoding of the map of in[i].  Each 32-byte half is read little-endian with bit 255 cleared and need not be
 *     below p.  The map never fails: there is no status.  Constant time: no branch or address depends on the input.
 *     n = 0 is a no-op; a NULL buffer with n > 0 is ZKP_ERR_ARG; at most 2^31 - 1 outputs per call.  Timed under ZKP_K_DECODE.
 *     zkp_from_uniform_bytes takes host pointers and synchronises; zkp_from_uniform_bytes_dev takes device pointers (16-byte
 *     aligned), enqueues on the context's stream without synchronising, and may be recorded between zkp_ctx_capture_begin / _end. */
int zkp_from_uniform_bytes(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][64]*/, uint8_t* out /*[n][32]*/);
int zkp_from_uniform_bytes_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_in /*[n][64]*/, uint8_t* d_out /*[n][32]*/);
/*     N x { transcript.challenge_bytes(label, 64) ; from_uniform_bytes }, the `hash_to_group` of the reference's VRF example
 *     (tests/sig_and_vrf_example.rs:36-40), with the transcripts on the device: all N blobs must stand at one STROBE position
 *     (ZKP_ERR_ARG otherwise), and they are advanced in place exactly as merlin advances them.  Host pointers, synchronous.
 *     The squeeze is timed under ZKP_K_TRANSCRIPT, the map under ZKP_K_DECODE. */
int zkp_fused_hash_to_group(zkp_ctx* ctx, uint32_t N, uint8_t* transcripts /*[N][208]*/, const char* label, uint8_t* out /*[N][32]*/);
/*     The same for transcripts at any mix of STROBE positions. */
int zkp_fused_hash_to_group_ragged(zkp_ctx* ctx, uint32_t N, uint8_t* transcripts /*[N][208]*/, const char* label, uint8_t* out /*[N][32]*/);
/*     n x RistrettoPoint::hash_from_bytes::<Sha512>(message) (reference tests/zkp.rs:34): SHA-512 (FIPS 180-4) of each message,
 *     then from_uniform_bytes above.  The messages are a CSR batch: message i = msgs[offsets[i], offsets[i + 1]), of any length
 *     and at any byte offset.  Lengths are public: branches depend on them, never on message bytes.  One lane hashes one message,
 *     so a batch runs at the pace of its longest message.  n = 0 is a no-op; n > 2^31 - 1 is ZKP_ERR_ARG.  The SHA-512 stage is
 *     timed under ZKP_K_TRANSCRIPT, the map under ZKP_K_DECODE.
 *     zkp_hash_from_bytes_sha512 takes host pointers: offsets must be non-decreasing (ZKP_ERR_ARG otherwise, and for a NULL buffer);
 *     it uploads msgs[offsets[0], offsets[n]) and the offsets rebased to 0, and synchronises.
 *     zkp_hash_from_bytes_sha512_dev takes device pointers (d_offsets 8-byte aligned, d_out 16-byte aligned, d_msgs any alignment;
 *     d_msgs may be NULL when msgs_len = 0), enqueues on the context's stream and may be recorded between zkp_ctx_capture_begin /
 *     _end once the same call has run outside the capture.  It does not check d_offsets: every range is clamped to [0, msgs_len)
 *     and hi < lo is empty, so a bad offset gives a wrong point, never a read outside d_msgs.  d_out may point at a row of a fused
 *     flow's d_table, so that an instance point such as H is hashed in place ahead of zkp_fused_prove_dev / _batch_verify_dev. */
int zkp_hash_from_bytes_sha512(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, uint8_t* out /*[n][32]*/);
int zkp_hash_from_bytes_sha512_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_msgs, uint64_t msgs_len, const uint64_t* d_offsets /*[n+1]*/,
                                   uint8_t* d_out /*[n][32]*/);

/* (6) Scalars mod l, batched (curve25519_dalek::scalar::Scalar).  Every output is a canonical 32-byte little-endian scalar; an input
 *     documented as "any 32 bytes" is read as Scalar::from_bytes_mod_order reads it.  One lane per output; no branch or address depends
 *     on an operand.  n = 0 is a no-op; a NULL buffer with n > 0, or n > 2^31 - 1, is ZKP_ERR_ARG.  The plain forms take host pointers,
 *     upload, run, download and synchronise; the _dev forms take device pointers (32- and 64-byte elements 16-byte aligned), enqueue on
 *     the context's stream without synchronising and may be recorded between zkp_ctx_capture_begin / _end (zkp_sc_random_dev once the
 *     same call has run outside the capture: it draws into the workspace).  Timed under ZKP_K_SCALARS.
 *     zkp_sc_invert: out[i] = (in[i] mod l)^-1, 0 -> 0 (Scalar::invert); in = any 32 bytes; out may equal in.
 *     zkp_sc_from_wide: n x Scalar::from_bytes_mod_order_wide.
 *     zkp_sc_muladd: out[i] = a[i a_stride] b[i b_stride] + c[i c_stride] mod l.  A stride counts elements and is 1, or 0 for one scalar
 *       shared by all outputs (anything else is ZKP_ERR_ARG); c == NULL means + 0.  Operands are any 32 bytes; out may equal an operand
 *       of stride 1.
 *     zkp_sc_random: n x Scalar::random: out[i] = from_bytes_mod_order_wide(zkp_chacha20_block(key, i, nonce)), drawn on the device.
 *     zkp_sc_hash_from_bytes_sha512: n x Scalar::hash_from_bytes::<Sha512> over a CSR batch, with the arguments, offset checks, clamping
 *       and rebasing of zkp_hash_from_bytes_sha512 / _dev above (d_msgs of any alignment, d_offsets 8-byte aligned).  One kernel: the
 *       digest never reaches memory.  Branches depend on the message lengths only.  Timed under ZKP_K_TRANSCRIPT. */
int zkp_sc_invert(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][32]*/, uint8_t* out /*[n][32]*/);
int zkp_sc_invert_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_in /*[n][32]*/, uint8_t* d_out /*[n][32]*/);
int zkp_sc_from_wide(zkp_ctx* ctx, uint64_t n, const uint8_t* in /*[n][64]*/, uint8_t* out /*[n][32]*/);
int zkp_sc_from_wide_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_in /*[n][64]*/, uint8_t* d_out /*[n][32]*/);
int zkp_sc_muladd(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, const uint8_t* c, uint32_t c_stride,
                  uint8_t* out /*[n][32]*/);
int zkp_sc_muladd_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_a, uint32_t a_stride, const uint8_t* d_b, uint32_t b_stride, const uint8_t* d_c,
                      uint32_t c_stride, uint8_t* d_out /*[n][32]*/);
int zkp_sc_random(zkp_ctx* ctx, uint64_t n, const uint8_t key[32], uint64_t nonce, uint8_t* out /*[n][32]*/);
int zkp_sc_random_dev(zkp_ctx* ctx, uint64_t n, const uint8_t key[32], uint64_t nonce, uint8_t* d_out /*[n][32]*/);
int zkp_sc_hash_from_bytes_sha512(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, uint8_t* out /*[n][32]*/);
int zkp_sc_hash_from_bytes_sha512_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_msgs, uint64_t msgs_len, const uint64_t* d_offsets /*[n+1]*/,
                                      uint8_t* d_out /*[n][32]*/);

/* (7) Merlin operations on N transcripts, batched: what every flow starts from (the reference's KeyPair::sign, Signature::verify and
 *     KeyPair::vrf are `append_message(b"msg", message)` followed by a proof call, tests/sig_and_vrf_example.rs:86-160).  One lane runs one
 *     transcript through STROBE-128 (zkp_amd/csrc/strobe_lane.h); the transcripts may stand at any mix of positions and the messages may
 *     have any mix of lengths, so a batch runs at the pace of its longest message.  Branches and addresses depend on positions, the
 *     label's length and the messages' lengths, never on message or state bytes.  Timed under ZKP_K_TRANSCRIPT.
 *     Common rules: N = 0 is a no-op; a NULL buffer with N > 0, a NULL label, a label of more than 248 bytes or N > 2^31 - 1 is
 *     ZKP_ERR_ARG, and a failed check changes nothing.  Transcripts are 208-byte blobs (ZKP_TRANSCRIPT_BYTES of zkp_toolbox.h).
 *     zkp_transcripts_append_message: N x Transcript::append_message(label, message j) over a CSR batch, message j = msgs[offsets[j],
 *       offsets[j + 1]) at any byte offset; msgs may be NULL when every message is empty.  shared_initial != 0: ts[0] is the one blob
 *       every transcript starts from (Transcript::new(label) per proof) and all N blobs are written; shared_initial == 0: blob j is
 *       advanced in place.  Host pointers: offsets must not decrease, every length must fit 32 bits (merlin asserts that) and every
 *       position byte must be below 166, ZKP_ERR_ARG otherwise; uploads msgs[offsets[0], offsets[N]) with rebased offsets, synchronises.
 *     zkp_transcripts_append_message_dev: device pointers (blobs 16-byte aligned, d_offsets 8-byte aligned, d_msgs of any alignment and
 *       NULL when msgs_len = 0); enqueues on the context's stream without synchronising, uses no workspace, and may be recorded between
 *       zkp_ctx_capture_begin / _end.  d_ts_out may equal d_ts_in when shared_initial == 0; the shared blob must lie outside d_ts_out.
 *       It does not check d_offsets: every range is clamped to [0, msgs_len) and hi < lo is the empty message, and the clamped length is
 *       what gets framed: a bad offset gives another transcript, never a read outside d_msgs.  A blob whose position byte is 166 or
 *       more is corrupt and is copied through unchanged.
 *     zkp_transcripts_challenge_bytes / _dev: N x Transcript::challenge_bytes(label, out[j], len), the blobs advanced in place; len = 0 is
 *       allowed (the frame and the PRF's begin still advance the transcript; out may then be NULL).  The host-pointer form rejects a
 *       position byte of 166 or more; the _dev form (recordable, no workspace, d_out of any alignment) leaves such a blob as it is and
 *       writes zeros to its output.
 *     zkp_strobe_pos_after_append: pure arithmetic, no GPU: the position word pos | pos_begin << 8 | cur_flags << 16 of a transcript
 *       after one append_message with a label of label_len and a message of msg_len bytes, given its position word before.  A resident
 *       caller whose messages have one length passes d_ts_out straight to zkp_fused_prove_dev / _batch_verify_dev with it, without
 *       downloading a blob to learn strobe_pos.  (A position byte of 166 or more returns strobe_pos unchanged.)
 *     The rest of the reference's TranscriptProtocol (src/toolbox/mod.rs:165-228) and its prover's TranscriptRng (src/toolbox/prover.rs:78-89),
 *     for callers who write a protocol of their own out of the batched calls -- an OR-proof, another challenge structure.  The lane code
 *     has STROBE's KEY operation for them (flags A|C: it overwrites the state where ad XORs; its begin runs the permutation when the
 *     position is not 0, as PRF's does).  Same common rules; the host-pointer forms reject a position byte of 166 or more, the _dev forms
 *     (blobs 16-byte aligned, every other buffer of any alignment) enqueue without synchronising, use no workspace and are recordable.
 *     zkp_transcripts_witness_rng / _dev: for each of N transcripts, which are read and never written (build_rng clones):
 *         for k < m:  meta_ad(label); meta_ad(u32le(wlen), more); KEY(witness k)       rekey_with_witness_bytes(label, witness k)
 *         meta_ad("rng"); KEY(entropy j [32])                                         finalize(&mut rng)
 *         ZKP_RNG_SCALARS: count x { meta_ad(u32le(64)); PRF(64) }, each reduced with from_bytes_mod_order_wide -> out [N][count][32],
 *                          canonical (Scalar::random(&mut rng) per blinding)
 *         ZKP_RNG_BYTES:   meta_ad(u32le(count)); PRF(count) -> out [N][count]         one fill_bytes
 *       witnesses [N][m][wlen], one wlen per call; m = 0 and wlen = 0 are allowed (and are different transcripts: wlen = 0 still frames
 *       and keys); witnesses may be NULL when m * wlen = 0 and out when count = 0.  entropy [N][32] is the caller's: what the external
 *       RNG contributes.  The reference's label is "".  Any other mode is ZKP_ERR_ARG.  The _dev form writes zeros for a corrupt blob.
 *       Branches and addresses depend on positions, m, wlen, count and the label's length, never on witness, entropy or state bytes.
 *       The host-pointer form stages entropy and witnesses in the context's workspace and zeroes that region before it returns, on
 *       error paths too; the outputs' staging is not wiped (they are the caller's secrets as much as what it receives in `out`), nor is
 *       anything the HIP runtime stages for a copy from pageable memory.
 *     zkp_transcripts_challenge_scalars / _dev: N x get_challenge(label) = challenge_bytes(label, 64) reduced mod l in the same lane ->
 *       out [N][32], canonical; the blobs advance in place.  The _dev form leaves a corrupt blob as it is and writes zeros.
 *     zkp_transcripts_append_points / _dev: N x { append_message(kind, var_label); append_message("val", points[j][32]) } in one launch:
 *       kind = "ptvar" is append_point_var, "blindcom" append_blinding_commitment (any label works).  validate != 0 gives the validating
 *       forms: a row of 32 zero bytes (the identity's encoding) gets status[j] = 1 and its blob stays as it was, the reference's early
 *       return; nothing else is validated, as there.  status [N] (required when validate != 0, optional otherwise) gets 0 for every
 *       other row.  The _dev form leaves a corrupt blob as it is, with status 0.
 *     zkp_ctx_last_kernels names "k_strobe_witness_rng", "k_strobe_challenge_scalars" and "k_strobe_append_points". */
#define ZKP_RNG_SCALARS 0
#define ZKP_RNG_BYTES 1
int zkp_transcripts_append_message(zkp_ctx* ctx, uint32_t N, int shared_initial, uint8_t* ts /*[N][208]*/, const char* label,
                                   const uint8_t* msgs, const uint64_t* offsets /*[N+1]*/);
int zkp_transcripts_append_message_dev(zkp_ctx* ctx, uint32_t N, int shared_initial, const uint8_t* d_ts_in, uint8_t* d_ts_out,
                                       const char* label, const uint8_t* d_msgs, uint64_t msgs_len, const uint64_t* d_offsets /*[N+1]*/);
int zkp_transcripts_challenge_bytes(zkp_ctx* ctx, uint32_t N, uint8_t* ts /*[N][208]*/, const char* label, uint32_t len,
                                    uint8_t* out /*[N][len]*/);
int zkp_transcripts_challenge_bytes_dev(zkp_ctx* ctx, uint32_t N, uint8_t* d_ts /*[N][208]*/, const char* label, uint32_t len,
                                        uint8_t* d_out /*[N][len]*/);
uint32_t zkp_strobe_pos_after_append(uint32_t strobe_pos, uint64_t label_len, uint64_t msg_len);
int zkp_transcripts_witness_rng(zkp_ctx* ctx, uint32_t N, const uint8_t* ts /*[N][208]*/, const char* label, uint32_t m, uint32_t wlen,
                                const uint8_t* witnesses /*[N][m][wlen]*/, const uint8_t* entropy /*[N][32]*/, int mode, uint32_t count,
                                uint8_t* out /*[N][count][32] or [N][count]*/);
int zkp_transcripts_witness_rng_dev(zkp_ctx* ctx, uint32_t N, const uint8_t* d_ts /*[N][208]*/, const char* label, uint32_t m, uint32_t wlen,
                                    const uint8_t* d_witnesses /*[N][m][wlen]*/, const uint8_t* d_entropy /*[N][32]*/, int mode, uint32_t count,
                                    uint8_t* d_out /*[N][count][32] or [N][count]*/);
int zkp_transcripts_challenge_scalars(zkp_ctx* ctx, uint32_t N, uint8_t* ts /*[N][208]*/, const char* label, uint8_t* out /*[N][32]*/);
int zkp_transcripts_challenge_scalars_dev(zkp_ctx* ctx, uint32_t N, uint8_t* d_ts /*[N][208]*/, const char* label, uint8_t* d_out /*[N][32]*/);
int zkp_transcripts_append_points(zkp_ctx* ctx, uint32_t N, uint8_t* ts /*[N][208]*/, const char* kind, const char* var_label,
                                  const uint8_t* points /*[N][32]*/, int validate, uint8_t* status /*[N]*/);
int zkp_transcripts_append_points_dev(zkp_ctx* ctx, uint32_t N, uint8_t* d_ts /*[N][208]*/, const char* kind, const char* var_label,
                                      const uint8_t* d_points /*[N][32]*/, int validate, uint8_t* d_status /*[N]*/);

/* (8) Scalar * basepoint and Scalar * point, batched: `&sk * &RISTRETTO_BASEPOINT_TABLE` (PublicKey::from(&SecretKey), reference
 *     tests/sig_and_vrf_example.rs:58) and `&H * &x` (:112; the instance points of tests/zkp.rs and benches/dleq.rs) for n operands, each
 *     with the `compress()` that follows.  One launch per call: decode, walk and encode in one lane, no CSR index arrays.  Scalars are any
 *     32 bytes, reduced or not (the kernels reduce them mod l).  n = 0 is a no-op; a NULL buffer with n > 0, a stride other than 0 and 1, bad
 *     flags, n > 2^31 - 1 or a NULL context is ZKP_ERR_ARG with nothing written.  The zero scalar and the identity point give 32 zero bytes
 *     (status 0).  The plain forms take host pointers, upload, run, download and synchronise; the _dev forms take device pointers (16-byte
 *     aligned; d_status of any alignment), enqueue on the context's stream without synchronising and may be recorded between
 *     zkp_ctx_capture_begin / _end once the same call has run outside the capture.  Timed under ZKP_K_TERMS; zkp_ctx_last_kernels names
 *     "k_mul_base", "k_mul_pairs<true>" (ZKP_CT) or "k_mul_pairs<false>".
 *     zkp_mul_base: out[i] = encode((scalars[i] mod l) * B), B = the ristretto255 basepoint.  Always constant time, never fails: a walk of
 *       36 mixed additions over a fixed-base table of B that belongs to the context -- NOT one of the 64 slots of
 *       zkp_ctx_prepare_fixed_points: the call evicts nothing and changes no other call's schedule -- with the lane-crossbar look-up
 *       (ZKP_OPT_CT_LOOKUP 0).  The table (269 KB) is built at the first call, which therefore must not be inside a capture (ZKP_ERR_ARG).
 *     zkp_mul_points: out[i] = encode((scalars[i s_stride] mod l) * decode(points[i p_stride])); a stride counts elements and is 1, or 0
 *       for one operand shared by all outputs (as zkp_sc_muladd).  flags = ZKP_CT: a signed radix-16 ladder over the point's own eight
 *       multiples, every entry read for every digit and the wanted one kept with selects -- no branch, address or bank depends on a scalar,
 *       and a point that does not decode is walked as the identity, so the schedule does not depend on validity either; ZKP_VARTIME: the
 *       entry a digit names is loaded, zero digits load nothing.  status[i] = 1 and out[i] = 32 zero bytes where the point does not decode
 *       (decompress() == None), else 0.  out may equal points when p_stride = 1.
 *     Sizes (profiles/point_mul_bench.txt, one MI355X, stream time against zkp_msm_many on the job callers used to build; measured at 4,096,
 *       65,536, 262,144 and 2^20 outputs, nothing in between): zkp_mul_base is faster than zkp_msm_many after
 *       zkp_ctx_prepare_fixed_points([B]) at 4,096 and 65,536 (x 1.3, x 1.4), ties it at 262,144 and is NOT faster at 2^20 (x 0.84: an
 *       inverse square root per output where the term path encodes with one field inversion per 65,536); with B unregistered it is x 5 - 9
 *       faster at every size.  zkp_mul_points is faster at 4,096, 65,536 (x 1.1) and 262,144 (x 1.04, constant time) and equal at 2^20.
 *       The calls run these kernels at every size all the same -- the synchronous call is shorter at every measured size, no index arrays
 *       being uploaded -- and a caller bound by kernel time at 2^20 can keep zkp_msm_many_dev.  A zkp_mul_points call of more than
 *       262,144 outputs is launched in pieces that share the 302 MB of ladder tables. */
int zkp_mul_base(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars /*[n][32]*/, uint8_t* out /*[n][32]*/);
int zkp_mul_base_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_scalars /*[n][32]*/, uint8_t* d_out /*[n][32]*/);
int zkp_mul_points(zkp_ctx* ctx, uint64_t n, const uint8_t* scalars, uint32_t s_stride, const uint8_t* points, uint32_t p_stride, int flags,
                   uint8_t* out /*[n][32]*/, uint8_t* status /*[n]*/);
int zkp_mul_points_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_scalars, uint32_t s_stride, const uint8_t* d_points, uint32_t p_stride, int flags,
                       uint8_t* d_out /*[n][32]*/, uint8_t* d_status /*[n]*/);

/* (9) RistrettoPoint + RistrettoPoint, -, negation and iter().sum(), batched, each with the `compress()` that follows: how the instance points of
 *     real statements are formed (C2 - M of an ElGamal proof, N - r Y of an unblinding, a sum of public keys or of ciphertext components) without a
 *     253-bit walk per term, which is what a zkp_msm_many job with scalars 1 and l - 1 spends.  Neither call takes ZKP_CT / ZKP_VARTIME: there is no
 *     secret operand, and the code is free of branches on point values anyway (signs are selects, the addition formulas are the complete ones:
 *     a[i] == b[i], a[i] == -b[i] and identity operands are no special case).  Plain forms take host pointers, upload, run, download and synchronise;
 *     _dev forms take device pointers (points and out 16-byte aligned, the others naturally), enqueue on the context's stream and may be recorded
 *     between zkp_ctx_capture_begin / _end once the same call has run outside the capture.  A NULL context, a NULL buffer that the call would read or
 *     write, a stride other than 0 and 1 or an op other than the two is ZKP_ERR_ARG with nothing written.
 *     zkp_add_points: out[i] = encode(decode(a[i a_stride]) + decode(b[i b_stride])) (ZKP_PT_ADD) or the difference (ZKP_PT_SUB); a stride counts
 *       elements and is 1, or 0 for one operand shared by all outputs.  status[i] = 1 and out[i] = 32 zero bytes where either operand does not
 *       decode, else 0.  out may be a or b where that operand has stride 1 (a lane loads both rows before it stores).  Negation is ZKP_PT_SUB with
 *       a = 32 zero bytes at stride 0; doubling is a == b.  One launch ("k_add_pairs" under ZKP_K_REDUCE), one output per lane, no workspace.
 *     zkp_sum_points: out[i] = encode(sum over t in [off[i], off[i + 1]) of +- decode(points[pidx[t]])), off[0] = 0 and non-decreasing.
 *       pidx == NULL: term t is point t, and n_points must equal the number of terms.  neg == NULL: every term is added; else neg[t] != 0
 *       subtracts term t.  An empty range gives 32 zero bytes and status 0.  status[i] = 1 and out[i] = zeros where a point that sum i references
 *       does not decode; a bad point no term references flags nothing, and a flagged sum leaves its neighbours alone.  An index >= n_points is
 *       ZKP_ERR_ARG on the host-pointer form (as are decreasing offsets and off[0] != 0) and flags its sum on the _dev form, which does not read
 *       its arrays on the host; n_terms there is the length of pidx / neg and MUST equal d_off[n_sums], as in zkp_msm_many_dev: the launches are
 *       sized from it, and with any other value (or offsets that decrease) the outputs are unspecified -- every access stays inside the
 *       buffers all the same.  Every point is decoded once
 *       (ZKP_K_DECODE); the sums are then folded in levels over the term axis (ZKP_K_REDUCE): a lane folds zkp_sum_points_group() consecutive
 *       items, writes the sums that begin and end between its first and last run, and hands exactly two partial sums to the next level (its
 *       first and its last run; a lane with one run hands on that run and the identity), which is therefore 1/16 as wide; the level that is left with one group finishes, and one kernel encodes (ZKP_K_COMBINE).  The launches depend on n_terms and
 *       n_sums alone -- any mix of segment lengths, 2^20 sums of two terms or one sum of 2^20, runs the same plan.  No atomics, no lane waits
 *       for another, every output has one writer.  zkp_ctx_last_kernels(ZKP_K_REDUCE) names one entry per level launched: "k_sum_fold<true>"
 *       (the terms), then "k_sum_fold<false>@2", "@3", ... (the level number is appended to the kernel's name).
 *     zkp_sum_points_group: the items one lane folds per level (32); pure arithmetic, no context.
 *     Sizes (profiles/point_sum_bench.txt, one MI355X, stream time, min / median / max over the rounds, against zkp_msm_many on the same job with
 *       scalars 1, variable time, alternated in one process): pairs 0.170 / 0.170 / 0.173 ms at 4,096 outputs against 0.728 / 0.731 / 0.735,
 *       0.178 / 0.185 / 0.199 against 1.382 / 1.414 / 1.530 at 65,536, 2.64 / 2.72 / 2.86 against 21.8 / 21.9 / 22.7 at 2^20; sums of two terms
 *       0.435 / 0.447 / 0.457 against 0.729 / 0.731 / 0.734 at 4,096, 0.600 / 0.614 / 0.638 against 1.440 / 1.456 / 1.463 at 65,536, 3.33 / 3.38 / 3.42
 *       against 21.5 / 21.9 / 21.9 at 2^20; 64 sums of 1,024 terms 0.470 / 0.478 / 0.498 against 4.10 / 4.11 / 4.12, 1,024 such sums 1.41 / 1.43 / 1.44
 *       against 14.3; one sum of 65,536 terms 0.480 / 0.489 / 0.499 against 194 / 251 / 252, one of 2^20 terms 1.44 / 1.46 / 1.46 against 3,686 /
 *       3,806 / 3,977.  Faster beyond the spread at every measured shape.  For pairs zkp_add_points is the call to use: zkp_sum_points on 4,096
 *       pairs takes 0.45 ms (three dependent fold launches) where zkp_add_points takes 0.17 ms. */
#define ZKP_PT_ADD 0
#define ZKP_PT_SUB 1
int zkp_add_points(zkp_ctx* ctx, uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, int op,
                   uint8_t* out /*[n][32]*/, uint8_t* status /*[n]*/);
int zkp_add_points_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_a, uint32_t a_stride, const uint8_t* d_b, uint32_t b_stride, int op,
                       uint8_t* d_out /*[n][32]*/, uint8_t* d_status /*[n]*/);
int zkp_sum_points(zkp_ctx* ctx, uint32_t n_sums, const uint32_t* off /*[n_sums+1]*/, const uint32_t* pidx /*[T] or NULL*/,
                   const uint8_t* neg /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points,
                   uint8_t* out /*[n_sums][32]*/, uint8_t* status /*[n_sums]*/);
int zkp_sum_points_dev(zkp_ctx* ctx, uint32_t n_sums, const uint32_t* d_off /*[n_sums+1]*/, const uint32_t* d_pidx /*[n_terms] or NULL*/,
                       const uint8_t* d_neg /*[n_terms] or NULL*/, const uint8_t* d_points /*[n_points][32]*/, uint32_t n_points, uint32_t n_terms,
                       uint8_t* d_out /*[n_sums][32]*/, uint8_t* d_status /*[n_sums]*/);
uint32_t zkp_sum_points_group(void);

/* (10) Bounded discrete logarithms to the basepoint, batched: recover m from encode(m B), m < 2^bits -- the last step of exponential ElGamal
 *     (C2 - x C1 = m B), of a homomorphic tally or histogram and of an opened Pedersen value.  Baby-step / giant-step over canonical encodings:
 *     the context holds the encodings of i B, i < 2^baby_bits, and a point is searched by subtracting 2^baby_bits B per giant step.  Every
 *     candidate is walked as a HALF (the call first multiplies each point by (l + 1) / 2), so that its bytes come from the encoder of doubled
 *     points, whose one plain inversion is shared by a whole workgroup of candidates (Montgomery's trick as a product tree; zkp_dlog_group()
 *     candidates per inversion) instead of an inverse square root per candidate.
 *     VARIABLE TIME BY NATURE, unlike the constant-time calls of section 8: the duration of a call depends on the logarithms (small ones are
 *     found by the first launch, and a launch leaves early for finished points).  The logarithm of a SECRET must not be taken where timing is
 *     observable.  The call takes no ZKP_CT / ZKP_VARTIME flag.
 *     zkp_dlog_base: out[i] = the k in [0, 2^bits) with encode(k B) == points[i] and status[i] = ZKP_DLOG_FOUND; status[i] = ZKP_DLOG_INVALID and
 *       out[i] = 0 where the encoding does not decode; status[i] = ZKP_DLOG_NOT_FOUND and out[i] = 0 where no such k is in range.  k is unique
 *       when it exists (2^bits < l).  The identity (32 zero bytes) has logarithm 0.  bits is 1 .. 48: the cost of a point that is not found
 *       is 2^(bits - baby_bits) giant steps, and the cap keeps a mistyped bits from holding a shared GPU for hours (48 bits over a 2^22 table is
 *       2^26 steps per point); a call whose plan needs more than 65,536 step launches (n 2^(bits - baby_bits) above 2^41 or so) is refused as well:
 *       prepare a larger table or split the call.  n = 0 is a no-op; a NULL context, a NULL buffer with n > 0, n > 2^31 - 1 or bits outside
 *       1 .. 48 is ZKP_ERR_ARG with nothing written.  The plain form takes host pointers, uploads, runs, downloads and synchronises; the _dev
 *       form takes device pointers (d_points 16-byte, d_out 8-byte aligned), enqueues on the context's stream and may be recorded between
 *       zkp_ctx_capture_begin / _end once one call of the same size or one zkp_ctx_prepare_dlog has run outside the capture (the table and the
 *       workspace must exist).  A call on a context without a table builds the default size (2^16 rows) first.
 *     zkp_ctx_prepare_dlog: builds the context's baby-step table for baby_bits in 4 .. 22 (else ZKP_ERR_ARG): 32 bytes per row and 16 bytes of
 *       probe slots per row (an open-addressing table of 2^(baby_bits + 1) slots keyed by 32 bits of the encoding; a slot holds 32 more bits and
 *       the index; a match is confirmed against the 32 bytes of the row, and a refuted match does not end the probe).  The rows are computed on
 *       the device ("k_dlog_rows": a lane walks 16 consecutive i from (i0 / 2) B by adding (1/2) B, a workgroup encodes the doubles of one step of its
 *       lanes with one inversion), downloaded, and the slots are filled on the host and uploaded: no device atomics.  The table belongs to the
 *       context like the table of B behind zkp_mul_base: it takes none of the 64 slots of zkp_ctx_prepare_fixed_points and evicts nothing.
 *       Synchronous; ZKP_ERR_ARG inside a capture.  Preparing again with another size replaces the table (graphs captured over the old one are
 *       refused by zkp_graph_launch, as after a workspace growth); the same size again is a no-op.
 *     zkp_dlog_baby_bits: what the context holds; 0 = none yet (or a NULL context).
 *     zkp_dlog_group / zkp_dlog_chunk / zkp_dlog_slice_chunks(n): the plan, pure arithmetic: candidates per shared inversion (256), giant steps per
 *       work item (32), and the chunks per point one launch of a call of n points covers (max(1, 2^20 / n)).  A work item is (point, chunk), so
 *       one point with a large range fills the chip as well as 2^20 points with small ones; the launches follow each other on the stream in
 *       ascending order of k without host synchronisation.
 *     Timed under ZKP_K_DECODE ("k_dlog_prepare": decode and the halving, a variable-time radix-16 ladder) and ZKP_K_TERMS ("k_dlog_steps").
 *     Sizes (profiles/dlog_bench.txt, one MI355X, stream time, min / median / max over five rounds, table of 2^16 rows): a call whose range the
 *       table covers is the halving ladder and one step -- 0.77 / 0.81 / 0.95 ms for one point at 16 bits, 0.79 / 0.79 / 0.79 for 4,096, 0.87 / 0.89 /
 *       0.92 for 65,536; with giant steps a launch is never shorter than about 1.7 ms (a step of a workgroup is 16 barriers and one inversion, ~55 us):
 *       24 bits 2.42 / 2.49 / 2.60 ms for one point, 2.55 / 2.56 / 2.57 for 4,096, 9.60 / 9.65 / 9.70 for 65,536 uniform logarithms (9.60 / 9.62 / 9.67
 *       all small); 32 bits 2.56 / 2.64 / 2.77 ms for one point, 97.3 / 97.3 / 97.6 for 4,096 uniform (18.2 / 18.2 / 18.3 all small: later launches
 *       leave early, the first one does not), 2,162 for 65,536 uniform -- about 1.4 x 10^9 candidates per second; with 2^20 rows 4,096 points at
 *       32 bits take 9.72 / 9.74 / 9.75 ms: size the table to the range.  40 bits over 2^22 rows: 2.65 / 2.73 / 2.79 ms for one point, 379 / 380 /
 *       381 for 4,096.  Prepare: 1.1 ms (2^12 rows), 1.5 (2^16), 26 (2^20), 125 (2^22).  Against the route callers had (k B for every k in range and a
 *       row search; 4,096 points, synchronous call): 0.84 against 6.38 ms at 16 bits, 1.70 against 156 at 20, 2.62 against 3,965 at 24; beyond that
 *       its table does not fit.
 *       NOT faster than the host backend for small calls (synchronous call against zkp_basepoint_dlog_batch on 16 host threads): one point at
 *       16 / 24 / 26 bits takes 0.042 / 0.26 / 0.77 ms on the host against 0.88 / 2.60 / 2.61 ms here, 16 points at 16 bits 0.11 against 0.94, 113
 *       points 0.46 against 0.81; 227 points at 16 bits are the break-even (0.87 against 0.82).  zkp_toolbox.h routes calls up to that size to the
 *       host and says how.  4,096 points are x 18 (16 bits) and x 107 (24 bits) faster here. */
#define ZKP_DLOG_FOUND 0
#define ZKP_DLOG_INVALID 1
#define ZKP_DLOG_NOT_FOUND 2
int zkp_ctx_prepare_dlog(zkp_ctx* ctx, uint32_t baby_bits);
uint32_t zkp_dlog_baby_bits(zkp_ctx* ctx);
int zkp_dlog_base(zkp_ctx* ctx, uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, uint64_t* out /*[n]*/, uint8_t* status /*[n]*/);
int zkp_dlog_base_dev(zkp_ctx* ctx, uint64_t n, const uint8_t* d_points /*[n][32]*/, uint32_t bits, uint64_t* d_out /*[n]*/, uint8_t* d_status /*[n]*/);
uint32_t zkp_dlog_group(void);
uint32_t zkp_dlog_chunk(void);
uint32_t zkp_dlog_slice_chunks(uint64_t n);

/* (10, continued) ... to ANY base, and over SIGNED ranges: the amount sits on a generator G of the caller's (a second generator from
 *     hash-to-group, a per-election or per-asset generator, the value generator of a Pedersen scheme whose B carries the blinding), and net
 *     balances, score differences and tallies with retractions are signed.  The search is the one above -- the same kernels, which take their
 *     fixed-base table and their walk points as arguments -- over a SLOT: a table the context owns for one base.  ONE base per call; per-point
 *     bases are out of scope.
 *     zkp_ctx_prepare_dlog_point: builds slot `slot` (below ZKP_DLOG_SLOTS) for the base with encoding `base`: G's fixed-base table in the layout of
 *       the context's table of B ("k_decode_affine", "k_hot_bases", "k_hot_rows" over the one encoding), the rows encode(i G), i < 2^baby_bits
 *       (baby_bits 4 .. 22), their probe slots and the walk points (1/2) G and (2^baby_bits / 2) G, as zkp_ctx_prepare_dlog builds them for B.  The
 *       slots take none of the 64 slots of zkp_ctx_prepare_fixed_points, touch neither the context's own dlog table nor its table of B, and are
 *       freed with the context.  Synchronous; ZKP_ERR_ARG inside a capture.  The same base and size again is a no-op; anything else replaces the
 *       slot, and graphs recorded over a replaced or released slot are refused by zkp_graph_launch.  ZKP_ERR_ARG with the slot left as it was: a
 *       base that does not decode, the identity (32 zero bytes: every point is a multiple of any other element of the group, but of the
 *       identity only itself), slot >= ZKP_DLOG_SLOTS, baby_bits outside 4 .. 22, a NULL pointer.  A failed allocation is ZKP_ERR_OOM and leaves
 *       the slot empty.
 *     zkp_ctx_release_dlog_point: frees the slot (an empty one: no-op).  Synchronous; ZKP_ERR_ARG inside a capture.
 *     zkp_dlog_point_baby_bits: the slot's size, 0 = empty (or no such slot, or a NULL context).  zkp_dlog_point_base: the encoding the slot was
 *       built from (ZKP_ERR_ARG for an empty slot).  zkp_dlog_point_find: the slot that holds this base, or -1.  zkp_dlog_point_last_use: the
 *       context counts prepares and searches over its slots; this is the count at the slot's last one, 0 for an empty slot -- the slot with the
 *       smallest is the least recently used (what zkp_point_dlog_batch of zkp_toolbox.h replaces when no slot is free).
 *     zkp_dlog_point[_dev]: zkp_dlog_base[_dev] with the slot's G for B: the same meaning of out and status, the same checks and limits (bits
 *       1 .. 48, n <= 2^31 - 1, at most 65,536 step launches, n = 0 a no-op, nothing written on an argument error) and the same recording rules.
 *       An empty slot is ZKP_ERR_ARG: there is no default base to build.  A slot prepared with the encoding of B returns exactly what
 *       zkp_dlog_base returns.  flags = 0: k in [0, 2^bits).  flags = ZKP_DLOG_SIGNED: k in [-2^(bits - 1), 2^(bits - 1)), written to out as a
 *       two's-complement int64 in the uint64 row (bits = 1: {-1, 0}); any other bit is ZKP_ERR_ARG.  The signed search is the unsigned one on
 *       Q + 2^(bits - 1) G: the prepare step adds 2^(bits - 1) (G / 2) to the halved point -- one point per call, computed by "k_dlog_setup" from the
 *       slot's fixed-base table, not a ladder per lane -- and a hit k' is written as k' - 2^(bits - 1).
 *     LAUNCH ORDER of a signed call: the slices of the chunk axis go on the stream in ascending distance from the slice that starts at k = 0,
 *       not in ascending k', so small magnitudes of either sign are found by the first two launches.  zkp_dlog_slice_order(n_slices, flags, i) is the
 *       slice launched i-th, pure arithmetic: i when unsigned; when signed, z = n_slices / 2 first, then z - 1, z + 1, z - 2, ... and the rest
 *       of the longer side once the shorter one is used up -- a permutation of 0 .. n_slices - 1.  For slice z to start at k = 0 exactly, a signed
 *       call's slice length is zkp_dlog_slice_chunks_signed(n): zkp_dlog_slice_chunks(n) rounded down to a power of two (the chunks of a point
 *       are a power of two as well).  Nothing else differs: same work items, same kernels.
 *       Both counts are returned as size_t, the 64-bit return type this header uses (a slice index is a count of slices).
 *     Timed under ZKP_K_DECODE ("k_dlog_prepare", or "k_dlog_prepare<shift>" for a signed call: the same text with the one addition) and
 *       ZKP_K_TERMS ("k_dlog_steps").
 *     Sizes: profiles/dlog_point_bench.txt (CHANGELOG.md has the summary).  The search costs what zkp_dlog_base costs -- group operations do not
 *       depend on the base -- so everything said above holds, including where the device does NOT win: small calls belong on the host
 *       (zkp_point_dlog_batch routes them there by the rule measured on B), and the first call on a new base pays one table build on top. */
#define ZKP_DLOG_SLOTS 8
#define ZKP_DLOG_SIGNED 1
int zkp_ctx_prepare_dlog_point(zkp_ctx* ctx, uint32_t slot, const uint8_t base[32], uint32_t baby_bits);
int zkp_ctx_release_dlog_point(zkp_ctx* ctx, uint32_t slot);
uint32_t zkp_dlog_point_baby_bits(zkp_ctx* ctx, uint32_t slot);
int zkp_dlog_point_base(zkp_ctx* ctx, uint32_t slot, uint8_t out[32]);
int zkp_dlog_point_find(zkp_ctx* ctx, const uint8_t base[32]);
size_t zkp_dlog_point_last_use(zkp_ctx* ctx, uint32_t slot);
int zkp_dlog_point(zkp_ctx* ctx, uint32_t slot, uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, int flags, uint64_t* out /*[n]*/,
                   uint8_t* status /*[n]*/);
int zkp_dlog_point_dev(zkp_ctx* ctx, uint32_t slot, uint64_t n, const uint8_t* d_points /*[n][32]*/, uint32_t bits, int flags, uint64_t* d_out /*[n]*/,
                       uint8_t* d_status /*[n]*/);
size_t zkp_dlog_slice_order(uint64_t n_slices, int flags, uint64_t i);
uint32_t zkp_dlog_slice_chunks_signed(uint64_t n);

/* (11) Multiscalar sums with LONG segments, batched: a vector Pedersen commitment sum m_i G_i + r H (constant time, many commitments over one set
 *     of generators), a weighted tally sum w_k C_k, an aggregated key sum a_k X_k, a caller's own random linear combination.  zkp_msm_many was
 *     built for very many MSMs of 2 to 11 terms: after its term kernels one lane per MSM adds that MSM's products one after another, and with long
 *     segments that serial sum is the whole call (profiles/point_sum_bench.txt: one MSM of 2^20 terms 8.9 ms of terms and 3.4 s of sum).
 *     zkp_msm_segments: meaning, argument checks and results are those of zkp_msm_many -- out[i] = encode(sum over t in [off[i], off[i + 1]) of
 *       scalars[t] * decode(points[pidx[t]])), scalars any 32 bytes, ZKP_CT or ZKP_VARTIME; status[i] = 1 and 32 zero bytes where a referenced point
 *       does not decode (the neighbours are left alone), an empty range gives 32 zero bytes and status 0; bad flags, off[0] != 0, decreasing
 *       offsets and an index >= n_points (host-pointer form) are ZKP_ERR_ARG with nothing written -- and so are its bytes.  pidx == NULL: term t
 *       uses point t, as in zkp_sum_points, and n_points must equal the number of terms (else ZKP_ERR_ARG).
 *       The call runs zkp_msm_many's term path unchanged up to the products (decode, classification, comb tables, "k_terms_*" under ZKP_K_TERMS:
 *       terms on points registered with zkp_ctx_prepare_fixed_points keep their fixed-base walk) on the scalars as given -- nothing is halved, the
 *       shared-inversion encoder is not used -- and then folds the term axis in the levels of zkp_sum_points: "k_sum_fold_parts" (level 1: item j
 *       is the product of term j, its bad flag the decode status of point pidx[j], an index at or beyond n_points flags the sum), then
 *       "k_sum_fold<false>@2", "@3", ... (ZKP_K_REDUCE), and k_sum_encode (ZKP_K_COMBINE).  The launch shapes follow from n_terms and n_msm alone;
 *       no atomics, one writer per output, every index that reaches memory is below its array's length whatever off and pidx hold.
 *       THE FOLD HAS NO BRANCH, ADDRESS OR TRIP COUNT THAT DEPENDS ON A SCALAR: it reads products, offsets and indices, and the segment structure
 *       (off, pidx, n_points) is public, as it is for zkp_msm_many.  What ZKP_CT promises is therefore what the term kernels promise.
 *       The _dev form takes device pointers (scalars, points, out 16-byte aligned), inspects no device array on the host, synchronises nowhere,
 *       sizes its workspace up front and may be recorded between zkp_ctx_capture_begin / _end once the same call has run outside the capture;
 *       n_terms MUST equal d_off[n_msm] (see zkp_sum_points_dev).
 *     NOT the call for short segments (zkp_msm_many's shared-inversion encoder wins there; zkp_toolbox.h routes by the longest segment) and NOT
 *       for one long variable-time MSM with an own point per term: zkp_msm_optional's bucket method does a fraction of the point operations.
 *     Sizes (profiles/msm_segments_bench.txt, one MI355X, stream time, min / median / max over the rounds, against zkp_msm_many on the same job,
 *       alternated in one process; variable | constant time): 64 segments of 1,024 terms 1.282 / 1.290 / 1.315 ms against 4.173 / 4.194 / 4.204 | 1.435 / 1.446 / 1.452 against 4.326 / 4.355 / 4.390; 1,024 such segments 12.63 / 12.64 / 12.66 ms against 15.87 / 15.96 / 15.98 | 13.97 / 14.04 / 14.04 against 17.23 / 17.29 / 17.31; one segment of
 *       65,536 terms 1.285 / 1.294 / 1.313 ms against 194.5 / 239.6 / 251.4 | 1.430 / 1.449 / 1.484 against 194.7 / 213.7 / 239.9; one of 2^20 terms 12.95 / 12.99 / 13.02 ms against 3403 / 3444 / 3525 | 14.40 / 14.45 / 14.47 against 3538 / 3810 / 3820; 16 segments of 65,536 terms over 65,536 shared points 6.233 / 6.272 / 6.405 ms against 222.6 / 266.4 / 266.5 | 5.599 / 5.601 / 5.602 against 247.8 / 255.7 / 265.6.  Faster beyond the spread
 *       at every one of these shapes, stream and synchronous call: the call is zkp_msm_many's term time plus 0.35 to 0.75 ms of fold.
 *       NOT faster on short segments (4,096 and 65,536 MSMs of 2, 11, 32 and 128 terms: fold against msm_many, ms, medians, variable time -- 4,096 x 2: 1.086 against 0.747; 4,096 x 11: 1.176 against 0.834; 4,096 x 32: 1.920 against 1.562; 4,096 x 128: 6.521 against 6.557; 65,536 x 2: 1.948 against 1.501; 65,536 x 11: 8.745 against 8.279; 65,536 x 32: 23.45 against 23.42; 65,536 x 128: 85.10 against 84.62), and NOT faster than zkp_msm_optional for one
 *       variable-time MSM with a point per term (65,536 terms: 1.248 ms against 0.834; 2^20 terms: 12.50 ms against 3.142): use those calls there. */
int zkp_msm_segments(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* off /*[n_msm+1]*/, const uint8_t* scalars /*[T][32]*/,
                     const uint32_t* pidx /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, int flags,
                     uint8_t* out /*[n_msm][32]*/, uint8_t* status /*[n_msm]*/);
int zkp_msm_segments_dev(zkp_ctx* ctx, uint32_t n_msm, const uint32_t* d_off /*[n_msm+1]*/, const uint8_t* d_scalars /*[n_terms][32]*/,
                         const uint32_t* d_pidx /*[n_terms] or NULL*/, const uint8_t* d_points /*[n_points][32]*/, uint32_t n_points,
                         uint32_t n_terms, int flags, uint8_t* d_out /*[n_msm][32]*/, uint8_t* d_status /*uint8 [n_msm]*/);

/* (12) Scalar sums, products and dot products over segments of any length, batched: dalek's `iter().sum()`, `iter().product()` and the inner
 *     product sum a_i b_i -- Lagrange coefficients prod m / (m - j), Shamir shares sum c_i j^i, powers j^i, the check sum lambda_j s_j == y, a
 *     verifier's acc_i = sum_k w_k m_ki.  zkp_sc_muladd writes one output per lane and has no reduction axis.
 *     zkp_sc_reduce: out[i] = the fold of the terms t in [off[i], off[i + 1]):
 *         ZKP_SC_SUM      sum  of a[ai(t)]               (an empty range: 0)
 *         ZKP_SC_PRODUCT  prod of a[ai(t)]               (an empty range: 1)
 *         ZKP_SC_DOT      sum  of a[ai(t)] * b[bi(t)]    (an empty range: 0)
 *       with ai(t) = aidx ? aidx[t] : t and likewise for b.  With a NULL index array the operand must have exactly T = off[n_out] rows.  Operands are
 *       any 32 bytes, read as Scalar::from_bytes_mod_order reads them; outputs are canonical; 0 and 1 are dalek's Sum and Product identities.  b, n_b
 *       and bidx belong to ZKP_SC_DOT and must be NULL / 0 / NULL otherwise.  out must not overlap an input.  Index lists may repeat and skip rows:
 *       one shared scalar, a matrix column, j^i as a product of i references to row j are all plain calls.
 *       n_out = 0 is a no-op.  ZKP_ERR_ARG with nothing written: a NULL context, a NULL buffer the call would read or write, an unknown op, more
 *       than 2^31 - 1 terms, and in the host-pointer form off[0] != 0, decreasing offsets, an index at or beyond its operand's length and a NULL
 *       index array with another operand length than T.
 *       The _dev form reads none of its arrays on the host; n_terms MUST equal d_off[n_out].  With another value, decreasing offsets or an index out
 *       of range the outputs that depend on the bad input are unspecified, every access still stays inside the buffers (indices are clamped, a
 *       term's segment is a binary search in d_off whose result is below n_out) and the outputs that do not reference the bad term are right.
 *       Scalars and d_out 16-byte aligned, offsets and indices 4-byte; queued on the context's stream without synchronising; may be recorded
 *       between zkp_ctx_capture_begin / _end once the same call has run outside the capture (it draws into the workspace).
 *     The plan (zkp_amd/csrc/sc_reduce.h) follows from n_terms and n_out alone: 2^20 sums of two terms and one sum of 2^20 terms make the same
 *       launches.  THE WORK UNIT IS A WORKGROUP: zkp_sc_reduce_group() (256) is both its number of lanes and the number of consecutive items of one
 *       level it folds, one item per lane.  Rows read in order arrive as 16 bytes per lane on consecutive addresses through an LDS tile; the
 *       stretches of the segments inside a unit are folded by a segmented scan with head flags over the lanes.  A stretch that begins and ends inside
 *       the unit is written to its output, the first and the last are handed on through the workspace as two items of the next level (the result
 *       does not depend on what the workspace held).  zkp_sc_reduce_levels(T) is the number of such launches: 1 up to 256 terms, 2 up to 32,768, 3
 *       up to 2^22.  One writer per output, no atomics, no lane waits for another workgroup.
 *       NO BRANCH, TRIP COUNT OR ADDRESS DEPENDS ON A SCALAR'S VALUE -- a zero factor does not end a product -- control flow follows off, the index
 *       arrays and the sizes only (profiles/scalar_reduce_ct_counters.txt).
 *       Timed under ZKP_K_SCALARS; zkp_ctx_last_kernels(ZKP_K_SCALARS) names one entry per level: "k_sc_fold<op, true>", "k_sc_fold<op, false>@2", ...
 *       k_sc_fold: 52 VGPRs (64 for products), no scratch, 18 KiB of LDS, 8 wavefronts per SIMD.
 *     Sizes (profiles/scalar_reduce_bench.txt, one MI355X, five rounds with the routes alternated in one process, min / median / max in ms; `stream` =
 *       HIP events around zkp_sc_reduce_dev on resident buffers, `call` = the synchronous host-pointer call, copies included, `host` = the host
 *       backend at 16 threads, `ints` = Python integers on the decoded rows):
 *       SUM, one segment of 2^20 terms: stream 0.054 / 0.056 / 0.073 (33.5 MB of terms in 0.056 ms: 604 GB/s, three launches; far below the memory
 *       system, the call is launch-bound at this size), call 0.764 / 0.767 / 0.788, host 1.648 / 1.715 / 1.751, ints 15.6.  SUM, 65,536 x 2: stream
 *       0.040, call 0.376, host 0.830, ints 18.2.  PRODUCT, one of 2^20: stream 0.171 / 0.172 / 0.175, call 0.888, host 4.874, ints 201.7; 4,096 x 32:
 *       stream 0.057, call 0.188, host 1.016, ints 25.1.  DOT, one of 2^20: stream 0.070 / 0.072 / 0.079, call 1.394, host 4.877, ints 93.7; 64 x
 *       1,024: stream 0.025, call 0.168, host 0.698, ints 5.6.  The Pedersen check as a matrix-vector job (K = 1,024 weights through aidx against
 *       1,025 columns): stream 0.084 / 0.090 / 0.101 against 3.703 / 3.861 / 4.016 for the loop of K zkp_sc_muladd_dev calls (x 43); call 1.096 / 1.129 /
 *       1.139 against 63.73 / 63.82 / 64.74 for the loop of K synchronous scalar_muladd calls (x 57) and 5.059 / 5.092 / 5.626 for the host backend.
 *     Where it does NOT win: the synchronous call is a bus transfer of 32 or 64 bytes per term and 32 per output for a few instructions of work.  In
 *       the sweep of 2^12 to 2^22 terms against the host backend at 16 threads it is ahead beyond the spread at 70 of 72 cells, but SUM of 2^22 terms
 *       in segments of 2 (2^21 outputs) is level with the host, 10.31 / 10.99 / 11.45 against 10.38 / 10.94 / 11.45, and one round of DOT at 2^14 x 32
 *       took 7.758 ms against 0.505; zkp_toolbox.h therefore routes SUM to the host by default.  Below 4,096 terms nothing is measured.  The host
 *       backend pays 0.37 to 0.45 ms for its 16 threads at every size up to 2^16 terms: one thread (not measured here) may well beat both. */
#define ZKP_SC_SUM 0
#define ZKP_SC_PRODUCT 1
#define ZKP_SC_DOT 2
int zkp_sc_reduce(zkp_ctx* ctx, int op, uint32_t n_out, const uint32_t* off /*[n_out+1]*/, const uint8_t* a /*[n_a][32]*/, uint32_t n_a,
                  const uint32_t* aidx /*[T] or NULL*/, const uint8_t* b /*[n_b][32] or NULL*/, uint32_t n_b, const uint32_t* bidx /*[T] or NULL*/,
                  uint8_t* out /*[n_out][32]*/);
int zkp_sc_reduce_dev(zkp_ctx* ctx, int op, uint32_t n_out, const uint32_t* d_off /*[n_out+1]*/, const uint8_t* d_a /*[n_a][32]*/, uint32_t n_a,
                      const uint32_t* d_aidx /*[n_terms] or NULL*/, const uint8_t* d_b /*[n_b][32] or NULL*/, uint32_t n_b,
                      const uint32_t* d_bidx /*[n_terms] or NULL*/, uint32_t n_terms, uint8_t* d_out /*[n_out][32]*/);
uint32_t zkp_sc_reduce_group(void);              /* pure arithmetic, no context */
uint32_t zkp_sc_reduce_levels(uint32_t n_terms); /* fold launches a call of n_terms terms makes; 0 for 0 */

/* (13) Prefix sums and prefix products over segments, batched: the running value at EVERY term where (9), (11) and (12) return one value per segment.
 *     Tables of powers x^0 .. x^(t-1) -- the weights w^k of a random linear combination, the rows j^i of a Shamir or Feldman Vandermonde matrix,
 *     Horner points, the prefix products behind Montgomery's inversion trick -- and running sums of points: the tally after every ballot, cumulative
 *     balances, the multiples G, 2G, 3G, .. of a caller's own generator.  Without a scan these are T calls, or a fold over all T prefixes, which is
 *     quadratic (j^i as zkp_sc_reduce over "i references to row j" is t (t - 1) / 2 terms for t powers).
 *     The job is in CSR form, T = off[n_seg], every term belongs to exactly one segment.  For term t of segment s
 *         ZKP_SCAN_INCLUSIVE  out[t] folds the terms [off[s], t]
 *         ZKP_SCAN_EXCLUSIVE  out[t] folds the terms [off[s], t): the first row of a segment is the identity -- 0, 1, or 32 zero bytes.
 *       A scan never crosses a segment boundary; an empty segment owns no rows.  n_seg = 0 or T = 0 is a no-op.
 *     zkp_sc_scan: ZKP_SC_SUM or ZKP_SC_PRODUCT of a[ai(t)], ai(t) = aidx ? aidx[t] : t.  Operands are any 32 bytes, read as
 *       Scalar::from_bytes_mod_order reads them; outputs are canonical.  aidx may repeat and skip rows, as in zkp_sc_reduce: the exclusive product
 *       scan of t references to row j is the table j^0 .. j^(t-1).  ZKP_SC_DOT is ZKP_ERR_ARG: a running dot product is zkp_sc_muladd (the
 *       products a_t b_t) followed by a sum scan.  out must not overlap an input.
 *     zkp_scan_points: pidx, neg, n_points and the decode rules are those of zkp_sum_points; there is no ZKP_CT / ZKP_VARTIME flag (nothing here
 *       reads a scalar).  status[t] = 1 and out[t] is zeros where a point among the terms out[t] depends on does not decode: a bad point flags its
 *       own row (the next row in exclusive mode) and every later row of its segment, nothing before it and nothing in another segment.  The
 *       additions are the complete ones: P, P, P, .. gives P, 2P, 3P, .. and P, -P the identity, with no special case.
 *     ZKP_ERR_ARG with nothing written: a NULL context, a NULL buffer the call would read or write, an unknown op or mode, more than 2^31 - 1
 *       terms, and in the host-pointer forms off[0] != 0, decreasing offsets, an index at or beyond its operand's length and a NULL index array
 *       with another operand length than T.
 *       The _dev forms read none of their arrays on the host; n_terms MUST equal d_off[n_seg].  With another value, decreasing offsets or an index
 *       out of range the rows that depend on the bad input are unspecified, every access still stays inside the buffers (indices are clamped, a
 *       term's segment is a binary search in d_off whose result is below n_seg) and the rows that do not depend on the bad term are right.
 *       Scalars, points and d_out 16-byte aligned, offsets and indices 4-byte; queued on the context's stream without synchronising; may be
 *       recorded between zkp_ctx_capture_begin / _end once the same call has run outside the capture (it draws into the workspace).
 *     The plans (zkp_amd/csrc/sc_scan.h, point_scan.h) are REDUCE-THEN-SCAN over dependent launches and follow from n_terms alone.  Up-sweep: a
 *       unit hands on the fold of its last run and whether a segment begins inside it, one item per unit, level by level; the top level is one
 *       unit; down-sweep: a unit scans its items again, its carry goes into its first run when that run began in an earlier unit, and every prefix
 *       is written.  One writer per row, no atomics, NO LANE WAITS FOR ANOTHER WORKGROUP (no look-back, no spinning), and the result does not depend
 *       on what the workspace held.
 *       Scalars: the unit is zkp_sc_reduce's workgroup of zkp_sc_scan_group() (256) lanes, one item per lane, rows in and out through the LDS tile
 *       on consecutive addresses.  zkp_sc_scan_launches(T) = 2 L - 1: 1 up to 256 terms, 3 up to 65,536, 5 up to 2^24.  NO BRANCH, TRIP COUNT OR
 *       ADDRESS DEPENDS ON A SCALAR'S VALUE -- a zero factor does not end a product scan (profiles/scalar_scan_ct_counters.txt).  Timed under
 *       ZKP_K_SCALARS; zkp_ctx_last_kernels(ZKP_K_SCALARS) names one entry per launch: "k_sc_scan<op, true, false>@1" (terms, up),
 *       "k_sc_scan<op, false, false>@2", .., "k_sc_scan<op, false, true>@2" (down), "k_sc_scan<op, true, true>@1".
 *       Points: the unit is zkp_sum_points' lane with zkp_scan_points_group() (32) consecutive items.  zkp_scan_points_launches(T) = 2 L + 1: the
 *       decode ("k_decode_affine" under ZKP_K_DECODE), "k_pt_scan<terms, down>@level" (ZKP_K_REDUCE; 1 walk up to 32 terms, 3 up to 1,024, 5 up to
 *       32,768, 7 up to 2^20, 9 up to 2^25) and the encode, one lane and one inversion per row ("k_pt_scan_encode" under ZKP_K_COMBINE): the names
 *       of the three kinds number zkp_scan_points_launches(T).  Workspace: 160 bytes per term and 112 per point.
 *       k_sc_scan: 50 to 54 VGPRs (64 to 68 for products), no scratch, 18 KiB of LDS.  The point scan encodes with the body behind k_sum_encode, one
 *       inversion per row; the shared-inversion encoder of doubled points (dlog.h) was not built or measured.
 *     Sizes (profiles/scan_bench.txt, one MI355X, five rounds with the routes alternated in one process, min / median / max in ms; `stream` = HIP
 *       events around the _dev call on resident buffers, `call` = the synchronous host-pointer call, copies included, `host` = the host backend at 16
 *       threads, `folds` = what callers had before: every prefix as a segment of its own in one zkp_sc_reduce / zkp_sum_points job):
 *       SUM, one segment of 2^20 terms: stream 0.087 / 0.090 / 0.102 (five launches; 33.5 MB read twice and written once: 1.1 TB/s), call 4.623, host
 *       5.045.  SUM, 64 x 1,024: stream 0.030 against folds 0.804 (x 27), call 0.200 against 10.78 (x 54), host 1.045.  PRODUCT (exclusive: tables of
 *       powers), one segment of 4,096: stream 0.053 against folds 0.988 (x 19), call 0.122 against 3.354 (x 28), host 0.935; 64 x 1,024: stream 0.060
 *       against 3.891 (x 64), call 0.229 against 13.38 (x 58), host 1.223; one of 2^20: stream 0.305 / 0.306 / 0.308, call 2.320, host 10.88.  From
 *       2^16 terms in one segment the folds are 2^31 terms and more and are not measured.
 *       Points, one segment of 4,096: stream 0.544 / 0.551 / 0.570 against 0.967 for the sums over all prefixes (8.4 million terms), call 0.640
 *       against 3.407, against 971.1 for the loop of 4,095 point_add calls and 4.278 for the host; 64 x 1,024: stream 0.779 against 2.238, call 0.978
 *       against 11.76, 218.4 (loop) and 30.23 (host); one of 2^20: stream 2.637 / 2.707 / 2.733 (decode 0.92, walks 0.80, encode 0.92), call 7.191,
 *       host 890.1.
 *     Where it does NOT win: segments of two -- 65,536 x 2 scalars: stream 0.039 (SUM) and 0.092 (PRODUCT) against 0.024 and 0.047 for the folds over the
 *       98,304 prefix terms, which are one launch where the scan is three; points: stream 0.896 against 0.699, call 1.215 against 1.167 and against
 *       0.442 for ONE point_add call, which is all a scan of pairs is.  Points in segments of 32 (4,096 x 32): stream 0.911 against 0.869 for the sums
 *       over all prefixes, the synchronous call still x 1.6 ahead.  The synchronous scalar call moves 32 bytes in and 32 bytes out per term for a few
 *       instructions of work: against the host backend SUM is level at 2^20 terms and behind at 2^22 in short segments (17.25 against 16.12), and
 *       PRODUCT at 2^20 terms took 6 to 34 ms from round to round against 9 to 14 on the host IN THE SWEEP, while the identical call in the shapes part
 *       of the same file took 2.302 / 2.320 / 2.347 ms: the slow rows are unexplained and were not reproduced -- they are no property of the call (SUM
 *       at that size reads 4.5 ms in both parts).  zkp_toolbox.h routes SUM to the host by default and, reading the sweep as it stands, PRODUCT below
 *       2^22 terms.  A point scan of 64 terms takes 0.37 ms as a synchronous call (seven launches at 4,096 terms, nine at 2^20). */
#define ZKP_SCAN_INCLUSIVE 0
#define ZKP_SCAN_EXCLUSIVE 1
int zkp_sc_scan(zkp_ctx* ctx, int op, int mode, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint8_t* a /*[n_a][32]*/, uint32_t n_a,
                const uint32_t* aidx /*[T] or NULL*/, uint8_t* out /*[T][32]*/);
int zkp_sc_scan_dev(zkp_ctx* ctx, int op, int mode, uint32_t n_seg, const uint32_t* d_off /*[n_seg+1]*/, const uint8_t* d_a /*[n_a][32]*/, uint32_t n_a,
                    const uint32_t* d_aidx /*[n_terms] or NULL*/, uint32_t n_terms, uint8_t* d_out /*[n_terms][32]*/);
uint32_t zkp_sc_scan_group(void);                   /* pure arithmetic, no context */
uint32_t zkp_sc_scan_launches(uint32_t n_terms);    /* kernel launches a scalar scan of n_terms terms makes; 0 for 0 */
int zkp_scan_points(zkp_ctx* ctx, int mode, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint32_t* pidx /*[T] or NULL*/,
                    const uint8_t* neg /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points, uint8_t* out /*[T][32]*/,
                    uint8_t* status /*[T]*/);
int zkp_scan_points_dev(zkp_ctx* ctx, int mode, uint32_t n_seg, const uint32_t* d_off /*[n_seg+1]*/, const uint32_t* d_pidx /*[n_terms] or NULL*/,
                        const uint8_t* d_neg /*[n_terms] or NULL*/, const uint8_t* d_points /*[n_points][32]*/, uint32_t n_points, uint32_t n_terms,
                        uint8_t* d_out /*[n_terms][32]*/, uint8_t* d_status /*uint8 [n_terms]*/);
uint32_t zkp_scan_points_group(void);
uint32_t zkp_scan_points_launches(uint32_t n_terms); /* decode, walks and encode of a point scan of n_terms terms; 0 for 0 */

/* (14) MANY variable-time multiscalar sums with LONG segments by the bucket method: dalek's RistrettoPoint::optional_multiscalar_mul for a batch of
 *     segments -- K independent random-linear-combination checks that each need their own verdict, the weighted tallies of K contests, the
 *     aggregated keys of K committees, a Feldman check per dealer.  zkp_msm_segments walks a ladder, comb or fixed-base table for EVERY term, so
 *     its work per term does not shrink with the segment's length; zkp_msm_optional runs Pippenger's bucket method, but is one MSM per call.
 *     zkp_msm_optional_many: meaning, argument checks and bytes are those of zkp_msm_many with ZKP_VARTIME, per segment -- out[i] = encode(sum over t
 *       in [off[i], off[i + 1]) of scalars[t] * decode(points[pidx ? pidx[t] : t])), scalars any 32 bytes; an empty segment gives the identity (32
 *       zero bytes) and status 0; status[i] = 1 and 32 zero bytes where a referenced point does not decode: a bad point flags the segments that
 *       reference it and no other.  pidx == NULL: a point per term, and n_points must equal the number of terms.  ZKP_ERR_ARG with nothing written
 *       for what zkp_msm_segments refuses: a NULL context or buffer, off[0] != 0, decreasing offsets, an index >= n_points, terms without scalars
 *       or points.  THERE IS NO FLAGS ARGUMENT: THE CALL IS VARIABLE TIME BY DEFINITION -- bucket indices, list lengths and addresses follow the
 *       scalars.  Public scalars only.
 *     The plan.  A RUN is zkp_msm_optional's kernels on K segments side by side ("k_pip_tile_hist" through "k_pip_combine", the batch index one more
 *       window coordinate), K MSMs of n slots each with n the longest segment of the run and the window width picked from n as zkp_msm_optional
 *       picks it.  "k_pip_prepare_csr<C>" reads segment seg(b) of the job for MSM b: lane i < len decodes its point and recodes its scalar as
 *       zkp_msm_optional does; a slot beyond the segment's length is PADDING -- the identity record and all-zero digits, which the histogram skips, so
 *       padding costs the prepare and sort passes their reads and no point addition.  "k_pip_rows" then takes the run's K rows and status words to
 *       out[seg(b)] and status[seg(b)].  K is bounded by K * windows <= 65535 and by a cap of 2^20 padded terms (K * n) per run, which also bounds
 *       the workspace; a segment longer than the cap is a run of its own.  Runs follow each other on the context's stream without host
 *       synchronisation in one workspace sized for the largest.  zkp_ctx_last_kernels(ZKP_K_DECODE) names every run with its shape and its place in
 *       the run order: "k_pip_prepare_csr<11>@K=16,n=65536,at=0".
 *       Runs are used for segments of MORE than zkp_msm_optional_many_min_segment() = 192 terms, the sizes the bucket kernels have ever run at;
 *       shorter work takes zkp_msm_many's term path in variable time and gives the same bytes.
 *     The host-pointer form reads off and plans: segments of 0 terms are written directly; segments of at most 192 terms go through the term
 *       path together as one job; the others are ordered by falling length into CLASSES -- the longest segment not yet placed and every segment
 *       more than half as long -- and each class is one sequence of runs, so no run pads a member by a factor of two or more.
 *     The _dev form reads no array on the host and cannot classify: it is ONE class.  All n_seg segments are padded to max_seg, THE CALLER'S PROMISE
 *       that no segment is longer, and chunked over K by the two limits; max_seg <= 192 takes the term path.  n_terms MUST equal d_off[n_seg].  A
 *       segment longer than max_seg leaves its own row unspecified; with that, with decreasing offsets or with an index out of range every access
 *       still stays inside the buffers (segment bounds and indices are clamped below their arrays' lengths) and the other rows are right.  Scalars,
 *       points and d_out 16-byte aligned, offsets and indices 4-byte; queued on the context's stream without synchronising; may be recorded between
 *       zkp_ctx_capture_begin / _end once the same call has run outside the capture.
 *     Sizes (profiles/msm_optional_many_bench.txt, one MI355X, stream time between HIP events, medians of five rounds, ms, routes alternated in one
 *       process, a point per term; the call | zkp_msm_segments with ZKP_VARTIME | a loop of zkp_msm_optional_dev per segment on resident buffers):
 *       16 x 65,536 terms 3.022 | 12.43 | 12.96; 64 x 16,384 3.625 | 12.44 | 35.21; 256 x 4,096 5.084 | 12.48 | 104.7; 1,024 x 1,024 5.301 | 12.39 |
 *       358.4 (zkp_msm_many: 16.62); 4,096 x 256 9.009 | 12.35 | - (zkp_msm_many: 12.74); a ragged mix of 1,000 segments of 200 to 2,000 terms and
 *       one of 2^18 7.631 | 16.02 | 354.8, its classes padding 1.35 M terms to 1.69 M slots (x 1.26); 16 x 65,536 over 65,536 shared points 2.975 |
 *       5.845.  Ahead beyond the spread of the rounds at every one of these, as a synchronous call too (16 x 65,536: 4.26 against 14.64 ms).
 *     WHERE IT DOES NOT WIN: one segment is zkp_msm_optional's time, because it is the same kernels (2^20 terms: 3.139 against 3.109 ms); the time
 *       per term rises as the segments get shorter (2.9 ns at 65,536 terms a segment, 5.1 ns at 1,024, 8.6 ns at 256: every segment pays its own
 *       bucket tree and Horner tail); FEW segments of moderate length are a narrow launch whose floor is the Horner tail: 4 x 256, 4 x 1,024 and
 *       16 x 256 terms all take 0.37 to 0.39 ms (0.24 ms of it k_pip_combine) -- still ahead of the fold (0.97 to 1.03 ms) and of zkp_msm_many
 *       (1.6 to 4.0 ms) at every shape measured, 4 and 16 segments of 256, 1,024 and 4,096 terms included, so no measured shape has the call
 *       behind; nothing is measured between 193 and 255 terms.
 *     What padding costs: no point addition (histogram and scatter skip magnitude 0: nothing is summed for bin 0), only the prepare and sort
 *       passes' work on the extra slots.  Every segment padded to twice its length (_dev, max_seg = 2 x length): x 1.16 at 64 x 16,384 (3.32 ->
 *       3.83 ms), x 1.21 at 1,024 x 1,024 (5.00 -> 6.05), x 1.10 at 4,096 x 256 (8.58 -> 9.47).
 *     The run cap: equal-length jobs of 2^21 terms at caps 2^21 / 2^20 / 2^19 / 2^18 / 2^17 / 2^16 (1, 2, 4, 8, 16, 32 runs), ns per term: 32 x 65,536
 *       2.75 / 2.90 / 3.48 / 4.81 / 7.19 / 12.39; 128 x 16,384 3.16 / 3.31 / 3.84 / 4.40 / 6.46 / 10.46; 512 x 4,096 4.65 / 4.74 / 5.06 / 5.61 /
 *       6.76 / 9.70; 2,048 x 1,024 5.00 / 4.78 / 4.93 / 5.41 / 6.57 / 9.06 -- level down to 2^20, which is the cap, and worse with every halving
 *       below it.
 *     zkp_ctx_last_timing on a call of more than seven runs: see there (the total spans the call; the per-kind split lumps the tail). */
int zkp_msm_optional_many(zkp_ctx* ctx, uint32_t n_seg, const uint32_t* off /*[n_seg+1]*/, const uint8_t* scalars /*[T][32]*/,
                          const uint32_t* pidx /*[T] or NULL*/, const uint8_t* points /*[n_points][32]*/, uint32_t n_points,
                          uint8_t* out /*[n_seg][32]*/, uint8_t* status /*[n_seg]*/);
int zkp_msm_optional_many_dev(zkp_ctx* ctx, uint32_t n_seg, const uint32_t* d_off /*[n_seg+1]*/, const uint8_t* d_scalars /*[n_terms][32]*/,
                              const uint32_t* d_pidx /*[n_terms] or NULL*/, const uint8_t* d_points /*[n_points][32]*/, uint32_t n_points,
                              uint32_t n_terms, uint32_t max_seg, uint8_t* d_out /*[n_seg][32]*/, uint8_t* d_status /*uint8 [n_seg]*/);
uint32_t zkp_msm_optional_many_min_segment(void);   /* 192: runs are used above it; pure arithmetic */

/* Timing of the last *_dev / host call on this context, measured with HIP events on the stream the
 * kernels were launched on.  kernel_ms[] is indexed by ZKP_K_*; returns the number of entries. */
enum {
  ZKP_K_DECODE = 0,      /* ristretto decode (+ affine-niels conversion, digit extraction)       */
  ZKP_K_TERMS = 1,       /* per-term scalar multiplication (small-MSM path)                       */
  ZKP_K_REDUCE = 2,      /* per-MSM sum of partials + compress                                    */
  ZKP_K_SORT = 3,        /* Pippenger: histogram + scan + scatter; small-MSM path: term classification    */
  ZKP_K_BUCKET = 4,      /* Pippenger: bucket accumulation                                        */
  ZKP_K_COMBINE = 5,     /* Pippenger: bucket reduction + window combination + compress           */
  ZKP_K_TRANSCRIPT = 6,  /* fused flows: batched Merlin/STROBE transcript programs                 */
  ZKP_K_SCALARS = 7,     /* fused flows: scalar arithmetic mod l (blindings, responses, coefficients, operand assembly) */
  ZKP_K_TABLES = 8,      /* small-MSM path: comb tables of the per-proof points (k_comb_tables*)                      */
  ZKP_K_COUNT = 9
};
/* A call records at most 32 timing marks.  One with more (zkp_msm_optional_many records four per run: more than seven runs) keeps moving its last
 * mark, so total_ms still spans the whole call, while kernel_ms files everything behind the 31st mark under the kind of the call's last mark. */
int zkp_ctx_last_timing(zkp_ctx* ctx, float* kernel_ms /*[ZKP_K_COUNT]*/, float* total_ms);
/* With profiling on: which VARIANT of a kind's kernel the last call launched, by the name rocprofv3 prints -- the kernels whose template
 * arguments depend on the call's size, flags or options (ZKP_K_TERMS: "k_terms_split<true, 16, true, false>", ZKP_K_TABLES:
 * "zkp::k_comb_tables_lane<16>" / "zkp::k_comb_tables_lane_nc<16>" (a call that vouches for reduced scalars: no carry tooth) / "zkp::k_tables_transcript_pc<16>", ZKP_K_TRANSCRIPT: "zkp::k_transcript_run" / "...run1", "zkp::k_strobe_append_csr" / "zkp::k_strobe_challenge" of section (7), ZKP_K_DECODE of the
 * large-MSM path: "k_pip_prepare<11>"); several names are joined with ';', kinds whose kernels never vary give "".  Writes a NUL-terminated
 * string of at most cap - 1 characters and returns the untruncated length.  Profiles and benchmarks label kernels from THIS, not from a
 * copy of the dispatch thresholds. */
int zkp_ctx_last_kernels(zkp_ctx* ctx, int kind, char* buf, size_t cap);
/* Enable (1) / disable (0) per-kernel event timing (off by default: events add launch gaps). */
int zkp_ctx_set_profiling(zkp_ctx* ctx, int enabled);

#ifdef ZKP_BUILD_TEST_HOOKS
/* ---- test-hook builds only (zkp_amd/libzkp_mi355x_testhooks.so, compiled with -DZKP_BUILD_TEST_HOOKS; the shipped library
 *      has none of this: no extra options, no k_noop / k_debug_quad / k_debug_row kernels, no scratch in its code object) ----------------
 * zkp_debug_quad_selftest: exercises the 4-lane cooperative point arithmetic used by the latency-bound kernels.  pairs =
 *   [n][2][32] encodings (P, Q); out = [n][4][32] = enc(2P), enc(P+Q), enc(P+Q) through Q's niels form, enc(P-Q) through the
 *   negated niels form.
 * zkp_debug_row_selftest: the same for the one-limb-per-lane arithmetic of the Horner tail (zkp_amd/csrc/rowfe.h): out = [n][3][32] = enc(2P),
 *   enc(P+Q), enc(2^11 P + Q).
 * zkp_ctx_set_option extras (measurement, profiles/r02_ab_experiments.txt blocks o and p):
 *   ZKP_TESTOPT_DUMMY_LAUNCHES = n empty kernels added to every zkp_fused_prove_dev call (what a launch costs a pipelined caller);
 *   ZKP_TESTOPT_GENERIC_CLASSIFIER = 1 sends the fused flows through the generic six-kernel term classifier instead of
 *   k_stmt_classify;
 *   ZKP_TESTOPT_PIP_MERGE picks the form of the Pippenger bucket merge whatever the call's size: 1 = a quad of lanes per bucket, 2 = one lane per
 *   bucket, 0 = by the call's bucket count again (same bytes either way);
 *   ZKP_TESTOPT_VOUCH_REDUCED = 1: constant-time zkp_msm_many calls vouch that every scalar is reduced mod l, as the fused prove flows do for
 *   their blindings: the term kernel skips the carry window and walks sign-folded scalars (same bytes for reduced scalars; anything else is the
 *   caller's error);
 *   ZKP_TESTOPT_PIP_RUN_CAP = the cap on the padded terms of one run of zkp_msm_optional_many (0: the library's), for measuring it;
 *   ZKP_TESTOPT_WAVE_CYCLES = 1 switches on a per-wavefront cycle recorder in the term kernel (s_memtime at entry and exit);
 * zkp_debug_wave_cycles copies out (and clears) up to cap records, [block][wavefront 0..3] = block class << 56 | cycles (class 1 =
 *   ladder, 2 = comb scan, 3 = grouped comb walk, 4 = fixed-base; 0 = no record): the timing side of the constant-time evidence.
 * zkp_debug_sha512: the SHA-512 stage of zkp_hash_from_bytes_sha512 alone (same arguments and checks): out = [n][64] digests.
 * zkp_debug_last_schedule: the size-driven choices the last call on ctx made, as "key=value" pairs separated by spaces (only the keys the
 *   call decided): batch_encode (k_encode_* against k_reduce_encode), enc_groups (k_encode_invert blocks), opt_pip (zkp_msm_optional: Pippenger
 *   against the term path), pip_c, pip_part, status_shared (batch verification's status words without memsets), lat_split, grouped, comb_min,
 *   ladder_interleave, riders, straus_lanes, straus_wins, tr_lanes, tr_steps, fuse_tt (tables + transcript in one launch), terms_split (the
 *   classified term path against one k_terms_r4 lane per term), ragged_classes, ragged_compiled, ragged_base and fused_plans (the _ragged calls:
 *   position classes, class programs compiled by this call, 1 if it built its position-free base plan, the size of the aligned plan cache), pip_merge
 *   (the bucket merge: 0 = a quad per bucket, 1 = a lane per bucket), pip_buckets (batches x windows x buckets per window, what pip_merge goes by) and
 *   no_carry (1 = the term kernel skipped the carry window: the fused prove flows, whose scalars are reduced mod l) and sign_fold (1 = its
 *   fixed-base blocks walked min(s, l - s) in 36 windows and negated the result where l - s was walked, and so did the grouped comb walk in its
 *   radix-16 digits; the comb scans and the constant-time ladder fold whenever no_carry is 1).  Writes a
 *   NUL-terminated string of at most cap - 1 characters and returns the untruncated length. */
int zkp_debug_quad_selftest(zkp_ctx* ctx, uint32_t n, const uint8_t* pairs /*[n][64]*/, uint8_t* out /*[n][128]*/);
int zkp_debug_row_selftest(zkp_ctx* ctx, uint32_t n, const uint8_t* pairs /*[n][64]*/, uint8_t* out /*[n][96]*/);
int zkp_debug_wave_cycles(zkp_ctx* ctx, uint64_t* out, uint32_t cap);     /* returns the number of records copied */
int zkp_debug_sha512(zkp_ctx* ctx, uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, uint8_t* out /*[n][64]*/);
int zkp_debug_last_schedule(zkp_ctx* ctx, char* buf, size_t cap);
/* zkp_debug_ragged_blocks: the class grouping the _ragged calls launch: idx [N] = proof indices sorted stably by class, blocks [cap][3] =
 * (class, first, count) per wavefront, classes in order of first appearance.  Returns the number of blocks. */
int zkp_debug_ragged_blocks(const uint8_t* transcripts, uint32_t N, uint32_t* idx, uint32_t* blocks, uint32_t cap);
/* zkp_debug_fill_workspace: leaves in the device workspace what earlier calls of any kind may have left there.  Grows the workspace to at least
 * min_bytes the way every call does (a captured graph goes stale exactly as after a larger call), sets every 32-bit word of ALL of it to `word` on
 * the context's stream and waits for both of the context's streams.  Plans, tables and options are untouched.  ZKP_ERR_ARG during a capture or
 * with a job pending.  Results never depend on it: tests/test_gpu_workspace_residue.py runs every layout behind word = 0 (what a fresh allocation
 * holds), 3 (both bits of the two-bit status words; a small counter) and 0xFFFFFFFF. */
int zkp_debug_fill_workspace(zkp_ctx* ctx, size_t min_bytes, uint32_t word);
/* zkp_debug_ws_bytes: the size of the device workspace as it stands (0 before the first call): grow-only, the largest call's need plus an eighth. */
size_t zkp_debug_ws_bytes(zkp_ctx* ctx);
/* zkp_debug_ws_count: waits for both of the context's streams, copies the whole workspace to the host and returns how often the len bytes at
 * `needle` occur in it (at any byte offset, overlapping occurrences counted).  What "zeroes the staging on every way out" promises can be read
 * back with it.  (size_t)ZKP_ERR_ARG for a NULL argument, len = 0, during a capture or with a job pending; (size_t)ZKP_ERR_HIP when a stream
 * reports an error or the copy fails; 0 while there is no workspace. */
size_t zkp_debug_ws_count(zkp_ctx* ctx, const uint8_t* needle, size_t len);
enum { ZKP_TESTOPT_DUMMY_LAUNCHES = 1001, ZKP_TESTOPT_GENERIC_CLASSIFIER = 1002, ZKP_TESTOPT_WAVE_CYCLES = 1003, ZKP_TESTOPT_PIP_MERGE = 1004, ZKP_TESTOPT_VOUCH_REDUCED = 1005, ZKP_TESTOPT_PIP_RUN_CAP = 1006 };
#endif

#ifdef __cplusplus
}
#endif
#endif /* ZKP_MI355X_H */

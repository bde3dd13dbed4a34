// Host execution of the engine entry points the host-transcript route of the toolbox uses (host_backend.cpp): the device headers
// fe25519.h / ge25519.h compiled for the host.  Signatures = zkp_mi355x.h (1), (2), (3) without the context.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../../include/zkp_mi355x.h"

namespace zkp {
namespace hostbk {
int msm_many(uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx, const uint8_t* points, uint32_t n_points, int flags,
             uint8_t* out, uint8_t* status);
// zkp_msm_segments (11): the results of msm_many (pidx == NULL: term t uses point t and n_points must be the number of terms), every argument
// checked before anything is written.  The term axis is cut into one stretch per thread (n_threads <= 0: one per core; never less than 16 terms
// each), so one long segment is the work of all threads where msm_many gives it to one.
int msm_segments_n(uint32_t n_msm, const uint32_t* off, const uint8_t* scalars, const uint32_t* pidx /*or NULL*/, const uint8_t* points, uint32_t n_points,
                   int flags, int n_threads, uint8_t* out, uint8_t* status);
// zkp_sc_reduce (12): segmented sums, products and dot products of scalars, every argument checked before anything is written.  The TERM axis is
// cut into one stretch per thread (n_threads <= 0: one per core; never less than 64 terms each); a segment longer than a stretch leaves one partial
// per stretch, combined at the end.
int sc_reduce_n(int op, uint32_t n_out, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx /*or NULL*/, const uint8_t* b /*or NULL*/,
                uint32_t n_b, const uint32_t* bidx /*or NULL*/, int n_threads, uint8_t* out);
// zkp_sc_scan / zkp_scan_points (13): segmented prefix sums and products of scalars and running sums of points, every argument checked before
// anything is written.  The threads share the TERM axis (n_threads <= 0: one per core; never less than 64 terms each): each scans its stretch from
// the identity, the stretch totals are scanned serially, and each thread fixes up its first run -- the rows before the first segment that begins
// inside its stretch (scalars: one operation per row; points: the rows are walked again from the carry, so a row is encoded once).
int sc_scan_n(int op, int mode, uint32_t n_seg, const uint32_t* off, const uint8_t* a, uint32_t n_a, const uint32_t* aidx /*or NULL*/, int n_threads,
              uint8_t* out /*[T][32]*/);
int point_scan_n(int mode, uint32_t n_seg, const uint32_t* off, const uint32_t* pidx /*or NULL*/, const uint8_t* neg /*or NULL*/, const uint8_t* points,
                 uint32_t n_points, int n_threads, uint8_t* out /*[T][32]*/, uint8_t* status /*[T]*/);
int msm_optional(uint64_t n, const uint8_t* scalars, const uint8_t* points, uint8_t out_point[32], int* status);
int decode_check(uint64_t n, const uint8_t* points, uint8_t* status);
int from_uniform_bytes(uint64_t n, const uint8_t* in /*[n][64]*/, uint8_t* out /*[n][32]*/);      // zkp_from_uniform_bytes (5)
// zkp_hash_from_bytes_sha512 (5): message i = msgs[offsets[i], offsets[i + 1]) clamped to [0, offsets[n]); the caller has checked the offsets
int hash_from_bytes_sha512(uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, uint8_t* out /*[n][32]*/);
// zkp_sc_* (6): the caller has checked pointers and strides; a slice of a call is a call of its own (strided operands advanced by the caller)
void sc_invert_n(uint64_t n, const uint8_t* in /*[n][32]*/, uint8_t* out /*[n][32]*/);
void sc_from_wide_n(uint64_t n, const uint8_t* in /*[n][64]*/, uint8_t* out /*[n][32]*/);
void sc_muladd_n(uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, const uint8_t* c /*or NULL*/, uint32_t c_stride,
                 uint8_t* out /*[n][32]*/);
void sc_hash_sha512_n(uint64_t n, const uint8_t* msgs, const uint64_t* offsets /*[n+1]*/, uint8_t* out /*[n][32]*/);
// zkp_mul_base / zkp_mul_points (8): the caller has checked pointers, strides and flags; a slice of a call is a call of its own (strided
// operands advanced by the caller).  mul_base_n is always constant time; mul_points_n with ZKP_CT keeps masked look-ups and skips no digit.
void mul_base_n(uint64_t n, const uint8_t* scalars /*[n][32]*/, uint8_t* out /*[n][32]*/);
void mul_points_n(uint64_t n, const uint8_t* scalars, uint32_t s_stride, const uint8_t* points, uint32_t p_stride, int flags, uint8_t* out /*[n][32]*/,
                  uint8_t* status /*[n]*/);
// zkp_add_points / zkp_sum_points (9): the caller has checked pointers, strides, op, offsets and indices; a slice of a call is a call of its own.
// sum_points_n: off holds ABSOLUTE term numbers (off[0] need not be 0, so a range of sums is off + lo, out + 32 lo, status + lo with pidx / neg /
// points unchanged); sums of more than skip_longer_than terms are left alone (neither out nor status written): the caller splits those with
// sum_points_partial -- the sum of the terms [t_lo, t_hi) as four canonical field elements X, Y, Z, T and a bad flag -- and sum_points_finish,
// which adds n partial sums and encodes.
constexpr size_t SUM_PARTIAL_BYTES = 129;
void add_points_n(uint64_t n, const uint8_t* a, uint32_t a_stride, const uint8_t* b, uint32_t b_stride, int op, uint8_t* out /*[n][32]*/,
                  uint8_t* status /*[n]*/);
void sum_points_n(uint32_t n_sums, const uint32_t* off /*[n_sums+1]*/, const uint32_t* pidx /*or NULL*/, const uint8_t* neg /*or NULL*/,
                  const uint8_t* points, uint8_t* out /*[n_sums][32]*/, uint8_t* status /*[n_sums]*/, uint32_t skip_longer_than = 0xffffffffu);
void sum_points_partial(uint32_t t_lo, uint32_t t_hi, const uint32_t* pidx, const uint8_t* neg, const uint8_t* points, uint8_t partial[SUM_PARTIAL_BYTES]);
void sum_points_finish(uint32_t n, const uint8_t* partials /*[n][SUM_PARTIAL_BYTES]*/, uint8_t out[32], uint8_t* status);
// zkp_dlog_base (10): the caller has checked pointers, bits (1 .. 48) and baby_bits (4 .. 22).  dlog_halve decodes a point and multiplies it by
// (l + 1) / 2, once per point: half = four canonical field elements X, Y, Z, T; returns ZKP_DLOG_INVALID (half zeroed) where the encoding does not
// decode, ZKP_DLOG_NOT_FOUND (nothing searched yet) otherwise.  dlog_base_range searches the giant steps [j_lo, j_hi) of a halved point
// (k = j 2^baby_bits + i) and returns ZKP_DLOG_FOUND with *k, or ZKP_DLOG_NOT_FOUND in that range (*k = 0): ranges of one point are independent,
// which is how the toolbox spreads a few points with large ranges over its threads.  dlog_base_n does both for the whole range of each of n points.
// The baby table of a size is built at its first use (or by dlog_prepare_table) and kept for the process behind a mutex.
constexpr size_t DLOG_HALF_BYTES = 128;
void dlog_prepare_table(uint32_t baby_bits);
int dlog_halve(const uint8_t point[32], uint8_t half[DLOG_HALF_BYTES]);
int dlog_base_range(const uint8_t half[DLOG_HALF_BYTES], uint32_t bits, uint32_t baby_bits, uint64_t j_lo, uint64_t j_hi, uint64_t* k);
void dlog_base_n(uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, uint32_t baby_bits, uint64_t* out /*[n]*/, uint8_t* status /*[n]*/);
// zkp_dlog_point (10): the same to a base of the caller's and over signed ranges; the functions above are these with the encoding of B and
// is_signed = false.  The process keeps at most 8 tables keyed by (base encoding, baby_bits), least recently used out, behind the same mutex.
// dlog_point_decodes: whether an encoding is a base at all.  dlog_point_prepare_table returns ZKP_DLOG_INVALID for one that does not decode (every
// function below assumes one that does), else 0.
// dlog_point_shift: the point a signed call adds to every half, 2^(bits - 1) (G / 2), in the format of a half -- computed once per call.
// dlog_point_halve is dlog_halve plus that point (shift = NULL: unsigned).  dlog_point_range with is_signed walks its groups of giant steps in
// ascending distance from the group that starts at k = 0 (dlog_slice_order of dlog.h over the groups of the whole range, those outside
// [j_lo, j_hi) passed over) and returns k less the bias 2^(bits - 1) as a two's-complement int64.
bool dlog_point_decodes(const uint8_t base[32]);
int dlog_point_prepare_table(const uint8_t base[32], uint32_t baby_bits);
void dlog_point_shift(const uint8_t base[32], uint32_t bits, uint8_t shift[DLOG_HALF_BYTES]);
int dlog_point_halve(const uint8_t point[32], const uint8_t* shift /*[DLOG_HALF_BYTES] or NULL*/, uint8_t half[DLOG_HALF_BYTES]);
int dlog_point_range(const uint8_t base[32], const uint8_t half[DLOG_HALF_BYTES], uint32_t bits, uint32_t baby_bits, bool is_signed, uint64_t j_lo,
                     uint64_t j_hi, uint64_t* k);
void dlog_point_n(const uint8_t base[32], uint64_t n, const uint8_t* points /*[n][32]*/, uint32_t bits, uint32_t baby_bits, bool is_signed,
                  uint64_t* out /*[n]*/, uint8_t* status /*[n]*/);
}  // namespace hostbk
}  // namespace zkp

// Host-side launch entry points of the gfx950 kernels (implemented in *.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention.h"

namespace dlion {

// ---- optimizer (lion_kernels.hip)
// rounding (K0 and K2): 0 = round to nearest even, 1 = stochastic rounding of the bf16 parameter store with
// the 16 hash bits of (rkey, cbase + bit_off + e) per element; cbase = 8 * the bucket's byte offset
hipError_t launch_lion_local(int dt, const int64_t* seg, const int64_t* chunks, int64_t n_chunks, float decay,
                             float neg_lr, float b1, float omb1, float b2, float omb2, const float* gscale,
                             hipStream_t st, int rounding = 0, uint32_t rkey = 0, int64_t cbase = 0);
hipError_t launch_lion_encode(int dt, const int64_t* seg, const int64_t* chunks, int64_t n_chunks, uint8_t* bits,
                              float b1, float omb1, float b2, float omb2, int update_m, int stochastic, float rr,
                              uint64_t seed, uint32_t step, const float* gscale, hipStream_t st,
                              int64_t cbase = 0);  // stochastic: global coordinate of the bucket's first bit
// fused clip_grad_norm_: per-chunk sum of squares, then norm + clip coefficient on device
hipError_t launch_grad_sumsq(int dt, const int64_t* seg, const int64_t* chunks, int64_t n_chunks, float* partial,
                             hipStream_t st);
hipError_t launch_clip_coef(const float* partial, int64_t n, float max_norm, float* out, hipStream_t st);
hipError_t launch_lion_vote_apply(int dt, const int64_t* seg, const int64_t* chunks, int64_t n_chunks,
                                  const uint8_t* planes, int64_t plane_stride, const uint8_t* alive, int world,
                                  int mode, int tie, const uint8_t* neg, float decay, float neg_lr, const uint8_t* own,
                                  unsigned long long* agree, hipStream_t st, int rounding = 0, uint32_t rkey = 0,
                                  int64_t cbase = 0);
hipError_t launch_vote_reduce(const uint8_t* recv, int64_t nbytes, const uint8_t* alive, int world, int tie,
                              uint8_t* out, uint8_t* neg_out, unsigned long long* ties, hipStream_t st);
// average vote on the all-to-all path: out[P][nbytes] = bit planes of the live-voter count, P = bit_length(world)
hipError_t launch_vote_count(const uint8_t* recv, int64_t nbytes, const uint8_t* alive, int world, uint8_t* out,
                             unsigned long long* ties, hipStream_t st);

// ---- flash attention (attention.hip)
hipError_t launch_attn_fwd(const AttnArgs& a, int D, bool drop, hipStream_t st);
hipError_t launch_attn_bwd(const AttnArgs& a, int D, bool drop, hipStream_t st);

// ---- fused residual + dropout + LayerNorm/RMSNorm (norm_kernels.hip)
// backward: `parts` blocks (4 rows of C <= 1024, or one wide row, per block
// iteration); part is [parts][3][C]
hipError_t launch_add_norm_fwd(const void* x, const void* y, const void* bias, const void* gamma, const void* beta,
                               void* xo, void* h, float* mean, float* rstd, int64_t rows, int C, float eps, bool rms,
                               uint32_t seed, uint32_t thresh16, float inv_keep, hipStream_t st);
hipError_t launch_add_norm_bwd(const void* dh, const void* dxo_in, const void* xo, const void* gamma, const float* mean,
                               const float* rstd, void* dx, void* dy, float* part, int parts, int64_t rows, int C,
                               bool rms, uint32_t seed, uint32_t thresh16, float inv_keep, hipStream_t st);

// ---- bias + GELU, SwiGLU, RoPE, partial sums (elementwise_kernels.hip)
hipError_t launch_bias_gelu_fwd(const void* z, const void* b, void* h, int64_t rows, int N, bool exact,
                                hipStream_t st);
hipError_t launch_bias_gelu_bwd(const void* dh, const void* z, const void* b, void* dz, float* dbpart, int parts,
                                int64_t rows, int N, bool exact, hipStream_t st);
hipError_t launch_swiglu_fwd(const void* g, const void* u, void* h, int64_t rows, int64_t F, int64_t ld_in,
                             hipStream_t st);
hipError_t launch_swiglu_fwd_t(const void* g, const void* u, void* h, void* ht, int64_t rows, int64_t F,
                               int64_t ld_in, hipStream_t st);
hipError_t launch_swiglu_bwd_t(const void* dh, const void* g, const void* u, void* dgu, void* dgut, int64_t rows,
                               int64_t F, int64_t ld_in, hipStream_t st);
hipError_t launch_swiglu_bwd(const void* dh, const void* g, const void* u, void* dg, void* du, int64_t rows,
                             int64_t F, int64_t ld_in, int64_t ld_out, hipStream_t st);
hipError_t launch_rope(const void* x, const void* cos, const void* sin, void* y, int64_t rows, int T, int H, int D,
                       bool inverse, int64_t x_ld, int64_t y_ld, hipStream_t st);
// ---- per-head q/k RMSNorm + RoPE (qk_norm.hip); D in {64, 128}, heads [0, split) take gamma_a, the rest gamma_b
// y [rows, Hx, D] contiguous, rstd [rows, Hx]; x token stride x_ld
hipError_t launch_qk_norm_rope_fwd(const void* x, const void* gamma_a, const void* gamma_b, const void* cos,
                                   const void* sin, void* y, float* rstd, int64_t rows, int T, int Hx, int D,
                                   int split, float eps, int64_t x_ld, hipStream_t st);
// in place on g (dz with cos / sin, dy with both null); part [parts, 2, D]: part p sums the token rows
// [p rpp, min((p + 1) rpp, rows)), rpp = ceil(rows / parts)
hipError_t launch_qk_norm_rope_bwd(void* g, const void* x, const float* rstd, const void* gamma_a, const void* gamma_b,
                                   const void* cos, const void* sin, float* part, int parts, int64_t rows, int T,
                                   int Hx, int D, int split, int64_t g_ld, int64_t x_ld, hipStream_t st);
// out (+)= bf16(scale[0] * sum_s part[s]) (scale: optional device scalar)
hipError_t launch_sum_partials(const float* part, int S, int64_t n, int64_t ld, void* out, bool accumulate,
                               hipStream_t st, const float* scale = nullptr);
hipError_t launch_colsum(const void* x, float* part, int parts, int64_t rows, int N, hipStream_t st);
// out (+)= bf16(sum over every row of up to 16 fp32 stacks [rows_k, >= n] (row stride lds_k))
hipError_t launch_sum_partials_multi(const float* const* ptrs, const int64_t* rows, const int64_t* lds, int nseg,
                                     int64_t n, void* out, bool accumulate, hipStream_t st);
// the same over Y row groups: pass 1 into scratch fp32 [Y, n], pass 2 out (+)= bf16(scale * sum) --
// for narrow tall stacks (few column blocks); Y from sum_partials_split_factor (1 = not worth it)
int sum_partials_split_factor(int64_t n, int64_t total_rows);
// out [C, Rp] (16-bit elements) = x [R, C]^T (row stride ldx), output columns R..Rp-1 zero; Rp % 8 == 0
hipError_t launch_transpose_pad(const void* x, int64_t R, int64_t C, int64_t ldx, void* out, int64_t Rp,
                                hipStream_t st);
hipError_t launch_sum_partials_split(const float* const* ptrs, const int64_t* rows, const int64_t* lds, int nseg,
                                     int64_t n, int Y, float* scratch, void* out, bool accumulate, const float* scale,
                                     hipStream_t st);

// ---- bf16 GEMM C[M,N] = A[M,K] . B[N,K]^T with fused epilogue (gemm.hip)
// epi: 0 plain, 1 + bias, 2 aux = z, C = gelu_tanh(z + bias), 3 the same with erf GELU,
// 4 C = bf16(A.B^T) * gelu_tanh'(aux + bias) with aux an input and part [2 * ceil(M/256)][N]
// fp32 column sums of C (bias gradient partials), 5 the same with erf GELU; 6 / 7 as 2 / 3 but
// aux = bf16(gelu'(z + bias)) (output); 8 C = bf16(A.B^T) * aux with aux that derivative (input)
// and the part column sums of 4 (no bias).
// Needs K % 128 == 0, N % 8 == 0, leading dims % 8 == 0.
hipError_t launch_gemm_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias,
                          void* aux, int ldaux, int M, int N, int K, int epi, float* part, hipStream_t st);

// ---- token + position embedding with dropout, scaled gradient accumulation (embedding.hip)
hipError_t launch_embed_fwd(const int64_t* ids, const void* wte, const void* wpe, void* out, int64_t n, int C, int T,
                            int64_t V, uint32_t seed, uint32_t thresh16, float inv_keep, int32_t* err, hipStream_t st);
// error-flag bits (index_check / embed_fwd): OR-ed into err[0]
// (4 is the host's position_ids check, ops/fused.py; 8 a cache position outside [0, Tmax), decode.hip)
constexpr int kIndexErrEmbed = 1, kIndexErrLabel = 2, kIndexErrCache = 8;
hipError_t launch_index_check(const int64_t* ids, int64_t n, int64_t hi, int64_t ignore, int32_t* err, int code,
                              hipStream_t st);
// dwte / dwpe nullable; sid / perm = stably sorted ids and their positions (needed with dwte)
hipError_t launch_embed_bwd(const void* dx, const int64_t* sid, const int64_t* perm, void* dwte, void* dwpe, int64_t n,
                            int C, int T, int64_t V, int pos_accumulate, uint32_t seed, uint32_t thresh16,
                            float inv_keep, hipStream_t st);
// y (+)= bf16(x * bf16(s[0])), s a device fp32 scalar
hipError_t launch_scale_acc(const void* x, const float* s, void* y, int64_t n, int accumulate, hipStream_t st);

// ---- weight-gradient GEMM (gemm_tn.hip): C[z][M,N] fp32 (+)= P^T Q over split z's rows of the
// nseg segments (P_i [seg_rows, >= M] ld ldp, Q_i [seg_rows, >= N] ld ldq; bf16, 16-byte aligned).
// Needs seg_rows % 128 == 0, M % 8 == N % 8 == 0, 1 <= splits <= nseg * seg_rows / 128, nseg <= 16.
// Cb non-null (splits == 1): C ignored, Cb [M, N] bf16 (+)= bf16(P^T Q) instead (the gradient itself).
hipError_t launch_gemm_tn(const void* const* P, const void* const* Q, int nseg, int64_t seg_rows, int ldp, int ldq,
                          float* C, int M, int N, int splits, bool accumulate, hipStream_t st, void* Cb = nullptr);

// diagnostic build of the plain GEMM with per-block timestamps (tools/gemm_stamps.py)
hipError_t launch_gemm_nt_stamped(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                                  unsigned long long* stamps, hipStream_t st);

// ---- LoRA adapter streams (lora.hip), bf16, r in {8, 16} (wide ranks below), widths % 8 == 0
// out[t, :r] = scale * drop(in)[t, :] . w^T, w [r, K]; dropout when thresh16 > 0
hipError_t launch_lora_rows(const void* in, int64_t ldin, const void* w, void* out, int64_t rows, int K, int r,
                            float scale, uint32_t seed, uint32_t thresh16, float inv_keep, hipStream_t st);
// out [rows, N] = o + bf16(s * u . b^T), u [rows, r], b [N, r]
hipError_t launch_lora_up(const void* o, int64_t ldo, const void* u, const void* b, void* out, int64_t rows, int N, int r,
                          float s, hipStream_t st);
// part fp32 = yscale * per-row-range y^T g'; mode 0: g' = g, part [parts, N, r]; mode 1:
// g' = drop(g), part [parts, r, N], also dx = drop'(y . a) with a [r, N]; lora_cols_parts picks
// the range count
int lora_cols_parts(int64_t rows, int N);
hipError_t launch_lora_cols(const void* g, int64_t ldg, const void* y, const void* a, void* dx, float* part, int64_t rows,
                            int N, int r, int parts, int mode, float yscale, uint32_t seed, uint32_t thresh16,
                            float inv_keep, hipStream_t st);
// the same three streams for r in {32, 64, 128} (lora_wide.hip): MFMA forms of all three.  lora_cols_parts_wide
// picks the range count: min(ceil(1024 / ceil(N / 128)), rows / (2 r)) but at least 1, so that the fp32 partials
// never exceed the bytes of the g operand
bool lora_wide_rank(int r);
hipError_t launch_lora_rows_wide(const void* in, int64_t ldin, const void* w, void* out, int64_t rows, int K, int r,
                                 float scale, uint32_t seed, uint32_t thresh16, float inv_keep, hipStream_t st);
hipError_t launch_lora_up_wide(const void* o, int64_t ldo, const void* u, const void* b, void* out, int64_t rows, int N,
                               int r, float s, hipStream_t st);
int lora_cols_parts_wide(int64_t rows, int N, int r);
hipError_t launch_lora_cols_wide(const void* g, int64_t ldg, const void* y, const void* a, void* dx, float* part,
                                 int64_t rows, int N, int r, int parts, int mode, float yscale, uint32_t seed,
                                 uint32_t thresh16, float inv_keep, hipStream_t st);

// ---- 4-bit blockwise quantization of frozen weights (quant.hip); n % 64 == 0, 16-byte aligned
// q [n / 2] uint8 (first element of a pair in the high nibble), absmax [n / 64] fp32, code [16] fp32
hipError_t launch_quant4(int dt, const void* w, const float* code, uint8_t* q, float* absmax, int64_t n,
                         hipStream_t st);
hipError_t launch_dequant4(int dt, const uint8_t* q, const float* absmax, const float* code, void* out, int64_t n,
                           hipStream_t st);
// transposed: out [K, >= N] (row stride ldo, 16-bit dtypes) = W^T for W [N, K]; N % 64 == 0, K % 128 == 0
hipError_t launch_dequant4_t(int dt, const uint8_t* q, const float* absmax, const float* code, void* out, int N, int K,
                             int64_t ldo, hipStream_t st);

// ---- LM head cross-entropy (xent_kernels.hip)
// variant 0 = auto (DLION_XENT env override), 1 fp32-row, 2 streaming, 3/4/5 packed 16-bit row (256/512/1024 thr)
hipError_t launch_softmax_xent(int dt, void* logits, const int64_t* labels, int64_t n, int64_t vp, int v, float* loss,
                               int variant, hipStream_t st);
// label smoothing eps in [0, 1) and z-loss weight zeta >= 0 (kernels of their own, same variants):
// loss = lse - (1 - eps) x_y - eps mean(x) + zeta lse^2, logits <- (1 + 2 zeta lse) p - (1 - eps) onehot - eps / v
hipError_t launch_softmax_xent_opts(int dt, void* logits, const int64_t* labels, int64_t n, int64_t vp, int v,
                                    float* loss, float eps, float zeta, int variant, hipStream_t st);

// ---- LM head scoring, forward only (lm_score.hip): read-only logits [n, vp], real columns j < v
// row_loss = lse - (1 - eps) x_y - eps mean(x) + zeta lse^2 (0 for a label outside [0, v)), row_lse = logsumexp,
// pred = lowest column of the row maximum, rank = #{x_j > x_y} + #{j < y : x_j == x_y} (-1 for an ignored row)
hipError_t launch_lm_score(int dt, const void* logits, const int64_t* labels, int64_t n, int64_t vp, int v, float eps,
                           float zeta, float* row_loss, float* row_lse, int* pred, int* rank, hipStream_t st);

// ---- LM head top-k, forward only (lm_topk.hip): read-only logits [n, vp], real columns j < v, 1 <= k <= 64, k <= v
// ids [n, k] = the first k columns under (greater value, then lower column; values compared as floats),
// values [n, k] = the stored logits there, lse [n] = logsumexp; one launch, no float atomics
hipError_t launch_lm_topk(int dt, const void* logits, int64_t n, int64_t vp, int v, int k, float* values, int* ids,
                          float* lse, hipStream_t st);

// ---- generation (decode.hip); bf16, D in {64, 128}
// One decode step's q [B, H, D] / k / v [B, Hkv, D] (row strides *_ld, heads contiguous): q and k normed (gains
// nullable, Qwen3) and rotated (tables [>= Tmax, D], nullable) at pos[b], clamped into [0, Tmax) with
// kIndexErrCache OR-ed into err[0]; q to q_out [B, H, D], k and v to cache[b, pos[b]] of the token-major caches
// (batch / token strides *_bs / *_ts, heads contiguous).
hipError_t launch_kv_append(const void* q, const void* k, const void* v, int64_t q_ld, int64_t k_ld, int64_t v_ld,
                            const int* pos, const void* cos, const void* sin, const void* q_gamma,
                            const void* k_gamma, float eps, void* q_out, void* k_cache, void* v_cache, int64_t kc_bs,
                            int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, int B, int H, int Hkv, int D, int Tmax,
                            int32_t* err, hipStream_t st);
// out [B, H D]: row b attends the keys [max(0, len - window), len) of its cache, len = min(kv_len[b], max_len,
// Tmax) (window 0: all).  splits blocks of chunk keys per (kv head, row), splits chunk >= min(window, max_len);
// fp32 partials part_m / part_l [B, H, splits], part_o [B, H, splits, D], reduced by a combine pass.
constexpr int kDecodeMaxSplits = 64;
hipError_t launch_decode_attention(const void* q, int64_t q_ld, const void* k_cache, int64_t k_bs, int64_t k_ts,
                                   const void* v_cache, int64_t v_bs, int64_t v_ts, const int* kv_len, float* part_m,
                                   float* part_l, float* part_o, void* out, int B, int H, int Hkv, int D, int Tmax,
                                   int max_len, int window, int splits, int chunk, float scale, hipStream_t st);

// ---- generation, T tokens per sequence (chunk_attention.hip); bf16, D in {64, 128}, 1 <= T <= kChunkMaxTokens
// kv_append over a chunk: q [B, T, H, D] / k / v [B, T, Hkv, D] (batch / token strides *_bs / *_ts, heads
// contiguous); token t of row b is normed / rotated at pos[b] + t and k, v written to cache[b, pos[b] + t] when
// t < n_new[b] (n_new nullable: T for every row, else clamped into [0, T]); a written token outside [0, Tmax)
// ORs kIndexErrCache into err[0] and is not written.  q_out [B, T, H, D] is written for every token.
constexpr int kChunkMaxTokens = 8;
hipError_t launch_kv_append_chunk(const void* q, const void* k, const void* v, int64_t q_bs, int64_t q_ts,
                                  int64_t k_bs, int64_t k_ts, int64_t v_bs, int64_t v_ts, const int* pos,
                                  const int* n_new, const void* cos, const void* sin, const void* q_gamma,
                                  const void* k_gamma, float eps, void* q_out, void* k_cache, void* v_cache,
                                  int64_t kc_bs, int64_t kc_ts, int64_t vc_bs, int64_t vc_ts, int B, int T, int H,
                                  int Hkv, int D, int Tmax, int32_t* err, hipStream_t st);
// out [B, T, H D]: query (b, t), t < n_new[b], attends the keys [max(0, len + t + 1 - window), len + t + 1) of
// its cache, len = kv_len[b] (the length before the chunk; len + n_new is clamped to min(max_len, Tmax)); other
// queries give zero rows.  q [B, T, H, D] contiguous.  splits blocks of chunk keys per (kv head, row), splits
// chunk >= min(window + T - 1, max_len); fp32 partials part_m / part_l [B, T, H, splits], part_o [B, T, H,
// splits, D], reduced by a combine pass.
hipError_t launch_chunk_attention(const void* q, const void* k_cache, int64_t k_bs, int64_t k_ts,
                                  const void* v_cache, int64_t v_bs, int64_t v_ts, const int* kv_len,
                                  const int* n_new, float* part_m, float* part_l, float* part_o, void* out, int B,
                                  int T, int H, int Hkv, int D, int Tmax, int max_len, int window, int splits,
                                  int chunk, float scale, hipStream_t st);

// ---- decode projections (skinny_gemm.hip); bf16, 1 <= M <= 16, K % 64 == 0, any N
// out[M, N] (row stride ldo) = x[M, K] (row stride ldx, 16-byte aligned rows) . w[N, K]^T (+ bias[N]), fp32
// accumulation, one rounding.  The 128-k steps of K are cut into `splits` runs of `per` steps ((splits - 1) per <
// steps <= splits per); splits > 1 needs part, fp32 [splits, M, N], and runs the combine pass.  The weight is
// contiguous bf16 [N, K], or quant.hip's 4-bit store of it (q, absmax per 64 elements, a 16-entry code); the
// two forms give the same bits for the same weight values.
constexpr int kSkinnyMaxM = 16;
constexpr int kSkinnyMaxSplits = 32;
hipError_t launch_skinny_gemm_nt(const void* x, int64_t ldx, const void* w, const void* bias, void* out, int64_t ldo,
                                 float* part, int M, int N, int K, int splits, int per, hipStream_t st);
hipError_t launch_skinny_gemm_w4(const void* x, int64_t ldx, const uint8_t* q, const float* absmax, const float* code,
                                 const void* bias, void* out, int64_t ldo, float* part, int M, int N, int K,
                                 int splits, int per, hipStream_t st);

}  // namespace dlion

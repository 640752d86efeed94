// Forward-only scoring of the LM head (gfx950): per row of a read-only [N, Vp]
// logit block the loss, the logsumexp, the top-1 token and the rank of the label.
//
// Nothing is written back to the matrix, so the row never has to live in
// registers: one streaming pass with 16-byte loads serves every vocabulary
// width at 2 B/logit for bf16 (the in-place loss kernels of xent_kernels.hip
// move 4).  One 512-thread block per row; every thread keeps
//   - an online max / sum-of-exp (softmax_xent_stream_kernel's form, rescaled
//     only when its maximum moves),
//   - the first column of its running maximum,
//   - the sum of the raw logits (label smoothing's uniform term),
//   - one counter: the columns that sort before the label's, by value first
//     (greater wins) and by column second (lower wins).  That count is the rank.
// The block combine is one DPP wave reduction per quantity and one LDS step.
// Ties follow torch.argmax: the lowest column among equal values, compared as
// floats (-0.0 == +0.0).
#include "common.h"

#include <climits>

namespace dlion {

constexpr int kScoreThreads = 512;
constexpr int kScoreUnroll = 4;  // 16-byte loads in flight per thread (two each for fp32)

// integer forms of common.h's DPP wave reductions (same lane patterns)
template <bool MIN>
__device__ __forceinline__ int dpp_step_i(int x, int sel) {
  int y;
  switch (sel) {  // the DPP control must be an immediate
    case 0: y = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false); break;   // quad_perm [1,0,3,2]
    case 1: y = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false); break;   // quad_perm [2,3,0,1]
    case 2: y = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, false); break;  // row_ror:4
    default: y = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false); break; // row_ror:8
  }
  return MIN ? min(x, y) : x + y;
}
template <bool MIN>
__device__ __forceinline__ int wave_reduce_i(int x) {
  x = dpp_step_i<MIN>(x, 0);
  x = dpp_step_i<MIN>(x, 1);
  x = dpp_step_i<MIN>(x, 2);
  x = dpp_step_i<MIN>(x, 3);
  const int r0 = __builtin_amdgcn_readlane(x, 0), r1 = __builtin_amdgcn_readlane(x, 16);
  const int r2 = __builtin_amdgcn_readlane(x, 32), r3 = __builtin_amdgcn_readlane(x, 48);
  return MIN ? min(min(r0, r1), min(r2, r3)) : (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ int wave_min_i(int x) { return wave_reduce_i<true>(x); }
__device__ __forceinline__ int wave_sum_i(int x) { return wave_reduce_i<false>(x); }

// 8 consecutive logits as they come from memory: one 16-byte vector (16-bit) or two (fp32)
template <int DT> struct Chunk8 {
  uint4 r;
  __device__ __forceinline__ void load(const uint16_t* p) { r = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void unpack(float (&f)[8]) const {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = Elem<DT>::to_f(static_cast<uint16_t>(j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xffffu));
  }
};
template <> struct Chunk8<kF32> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = reinterpret_cast<const float4*>(p)[0];
    b = reinterpret_cast<const float4*>(p)[1];
  }
  __device__ __forceinline__ void unpack(float (&f)[8]) const {
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
};

template <int DT>
__global__ void __launch_bounds__(kScoreThreads)
lm_score_kernel(const typename Elem<DT>::S* __restrict__ logits, const int64_t* __restrict__ labels, int64_t vp, int v,
                float eps, float zeta, float* __restrict__ row_loss, float* __restrict__ row_lse,
                int* __restrict__ pred, int* __restrict__ rank) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int W = kScoreThreads / 64;
  constexpr int U = kScoreUnroll;
  __shared__ float redm[W], reds[W], redx[W];
  __shared__ int redi[W], redr[W];
  const int64_t row = blockIdx.x;
  const S* x = logits + row * vp;
  const int64_t label = labels[row];
  const int lab = (label >= 0 && label < v) ? static_cast<int>(label) : -1;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // the label's logit comes straight from memory (one scalar load per row)
  const float xy = lab >= 0 ? E::to_f(x[lab]) : 0.f;

  float m = -INFINITY, sm = 0.f, xs = 0.f;
  int idx = tid * 8;  // first column of the running maximum: this thread's first column until a value beats -inf
  int rk = 0;

  auto score8 = [&](const Chunk8<DT>& c, int e) {
    float f[8];
    c.unpack(f);
    const int nv = v - e;  // real columns left, > 0
    if (nv < 8) {          // the one chunk per row that straddles v: padding counts for nothing
#pragma unroll
      for (int j = 1; j < 8; ++j) {
        xs += j < nv ? f[j] : 0.f;
        f[j] = j < nv ? f[j] : -INFINITY;
      }
      xs += f[0];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) xs += f[j];
    }
    // columns that sort before the label's: a greater value, or an equal one at a lower column
    const int rel = lab - e;
    if (rel >= 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) rk += f[j] >= xy ? 1 : 0;
    } else if (rel < 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) rk += f[j] > xy ? 1 : 0;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) rk += (f[j] > xy || (f[j] == xy && j < rel)) ? 1 : 0;
    }
    float cm = fmaxf(f[0], f[1]);
#pragma unroll
    for (int j = 2; j < 8; ++j) cm = fmaxf(cm, f[j]);
    if (cm > m) {  // rare after the first chunks; false for NaN
      int first = 7;
#pragma unroll
      for (int j = 6; j >= 0; --j) first = f[j] == cm ? j : first;
      idx = e + first;
      sm *= __expf(m - cm);
      m = cm;
    }
    if (m > -INFINITY) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm += __expf(f[j] - m);
    }
  };

  // columns at and past v are never read: v <= vp and vp % 8 == 0 keep every chunk inside the row
  for (int base = tid * 8; base < v; base += kScoreThreads * 8 * U) {
    Chunk8<DT> c[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int e = base + i * kScoreThreads * 8;
      if (e < v) c[i].load(x + e);
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int e = base + i * kScoreThreads * 8;
      if (e < v) score8(c[i], e);
    }
  }

  const float wm = wave_max_dpp(m);
  const float ws = wave_sum_dpp(m > -INFINITY ? sm * __expf(m - wm) : 0.f);
  const float wx = wave_sum_dpp(xs);
  const int wi = wave_min_i(m == wm ? idx : INT_MAX);
  const int wr = wave_sum_i(rk);
  if (lane == 0) {
    redm[wid] = wm;
    reds[wid] = ws;
    redx[wid] = wx;
    redi[wid] = wi;
    redr[wid] = wr;
  }
  __syncthreads();
  if (tid == 0) {
    float mx = redm[0];
#pragma unroll
    for (int w = 1; w < W; ++w) mx = fmaxf(mx, redm[w]);
    float sum = 0.f, sx = 0.f;
    int p = INT_MAX, r = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      sum += redm[w] > -INFINITY ? reds[w] * __expf(redm[w] - mx) : 0.f;
      sx += redx[w];
      p = redm[w] == mx ? min(p, redi[w]) : p;
      r += redr[w];
    }
    const float lse = mx + __logf(sum);
    const float uni = eps / static_cast<float>(v);
    float loss = lse - (1.f - eps) * xy + zeta * lse * lse;
    if (eps != 0.f) loss -= uni * sx;
    row_lse[row] = lse;
    row_loss[row] = lab >= 0 ? loss : 0.f;
    pred[row] = min(p, v - 1);
    rank[row] = lab >= 0 ? r : -1;
  }
}

// eps in [0, 1), zeta >= 0 and 0 < v <= vp, vp % 8 == 0 are checked by the binding
hipError_t launch_lm_score(int dt, const void* logits, const int64_t* labels, int64_t n, int64_t vp, int v, float eps,
                           float zeta, float* row_loss, float* row_lse, int* pred, int* rank, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(logits) % 16 != 0 || vp % 8 != 0 || v <= 0 || v > vp || n > INT_MAX)
    return hipErrorInvalidValue;
#define LM_SCORE(DT)                                                                                         \
  hipLaunchKernelGGL((lm_score_kernel<DT>), dim3(n), dim3(kScoreThreads), 0, st,                             \
                     static_cast<const typename Elem<DT>::S*>(logits), labels, vp, v, eps, zeta, row_loss,   \
                     row_lse, pred, rank)
  switch (dt) {
    case kF32: LM_SCORE(kF32); break;
    case kBF16: LM_SCORE(kBF16); break;
    case kF16: LM_SCORE(kF16); break;
    default: return hipErrorInvalidValue;
  }
#undef LM_SCORE
  return hipGetLastError();
}

}  // namespace dlion

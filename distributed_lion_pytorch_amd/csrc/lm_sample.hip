// Sampling from the LM head (gfx950): per row of a read-only [N, Vp] logit block one column drawn from the
// distribution left by temperature, top-k and top-p, with the row's logsumexp, the smallest surviving scaled logit
// and the number of survivors.  Forward only, one launch, nothing written to the logits.
//
//   s_j = fp32(x_j) * inv_t (one rounded multiply); NaN and -inf columns take part in nothing
//   top-k   column j survives iff fewer than k columns have a greater s (ties at the k-th value all survive)
//   top-p   over the top-k survivors: j survives iff the mass of the survivors with a greater s is < top_p
//           (equal values share their fate, the class of the maximum always survives)
//   draw    Gumbel-max: argmax over the survivors of s_j + g_j, g_j = -log(-log(u_j)), u_j = (n_j + 0.5) 2^-24,
//           n_j = mix32(mix32(j ^ key) + row * 0x9E3779B1 + 0x85EBCA6B) >> 8; the lowest column on ties
//
// One 512-thread block per row.  Every decision is made on integers, so no result depends on the order in which
// threads meet: values are compared through their monotone 32-bit keys, and probability mass is 32.32 fixed point,
// q_j = floor(exp(s_j - max) * 2^32) <= 2^32, summed in 64-bit integers (LDS ds_add_u64); at most 2^30 columns
// keep every sum below 2^62.
//   pass 1   online max / sum-of-exp over the row (the logsumexp) and every thread's greatest s.
//   bound    from the 512 thread maxima a value L below which nothing can survive: with top-k the k-th greatest
//            of them (lm_topk's bound); with top-p alone the greatest of them at and above which the maxima alone
//            already hold top_p of the row's mass in the same fixed point.  -inf when neither applies.
//   stage    one sweep appends the columns with s >= L to an LDS list of (s, column) pairs, 4096 at the most.
//            Everything after runs on that list; a row that leaves more in play (a flat row under top-p, a top_k
//            in the thousands, no filter at all) re-reads the row from L2 through the same filter instead.
//   select   radix select from the top, 8 bits a pass, on a 256-bin u64 histogram: weights 1 and target k give the
//            k-th value, weights q and target top_p * Z give top-p's floor, Z being the survivors' integer mass.
//            Digits that the storage type cannot set (bf16 and fp16 rows at temperature 1) are skipped.
//   draw     Gumbel scores for the survivors only, (score, column) reduced by max / lowest column; the same sweep
//            counts the survivors and takes their minimum.
#include "sampling.h"

#include <climits>

namespace dlion {

constexpr int kSampThreads = 512;
constexpr int kSampUnroll = 4;   // chunks of 8 logits in flight per thread
constexpr int kSampBins = 256;   // 8-bit digits
constexpr int kSampCap = 4096;   // staged (s, column) pairs: 32 KB of LDS

template <int DT> struct SampKey {  // bits of the fp32 image that the storage type can set
  static constexpr int bits = DT == kF32 ? 32 : (DT == kBF16 ? 16 : 24);
};

__device__ __forceinline__ uint32_t samp_key(float f) {  // monotone in f, -0.0 == +0.0
  uint32_t u = __float_as_uint(f);
  u = u == 0x80000000u ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// 32.32 fixed-point exp(s - m), s <= m; expf is the accurate one (the same s gives the same q in every pass)
__device__ __forceinline__ unsigned long long samp_mass(float s, float m) {
  return static_cast<unsigned long long>(expf(s - m) * 4294967296.f);
}

template <int DT>
__global__ void __launch_bounds__(kSampThreads)
lm_sample_kernel(const typename Elem<DT>::S* __restrict__ logits, int64_t vp, int v, float inv_t, int top_k,
                 double top_p, uint32_t key, int* __restrict__ ids, float* __restrict__ row_lse,
                 float* __restrict__ row_floor, int* __restrict__ row_kept) {
  using E = Elem<DT>;
  using S = typename E::S;
  using u64 = unsigned long long;
  constexpr int T = kSampThreads, W = kSampThreads / 64, U = kSampUnroll;
  __shared__ __attribute__((aligned(16))) float tmax[T];
  __shared__ u64 tq[T];
  __shared__ u64 hist[kSampBins];
  __shared__ u64 wtot[kSampBins / 64];
  __shared__ float cand_s[kSampCap];
  __shared__ int cand_c[kSampCap];
  __shared__ float redm[W], reds[W], redb[W], redf[W];
  __shared__ int redc[W], redn[W];
  __shared__ float row_stat[2];  // max, sum of exp(s - max)
  __shared__ u64 ctl64[2];       // target left inside the bucket, the survivors' mass
  __shared__ int ctl[2];         // staged pairs, bucket
  const int64_t row = blockIdx.x;
  const S* x = logits + row * vp;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // f(s[8], first column, real columns in the chunk); columns at and past v take part in nothing
  auto sweep = [&](auto&& f) {
    for (int base = tid * 8; base < v; base += T * 8 * U) {
      float c[U][8];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int e = base + i * T * 8;
        if (e < v) E::load8(x + e, c[i]);  // v <= vp and vp % 8 == 0 keep every chunk inside the row
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const int e = base + i * T * 8;
        if (e < v) {
#pragma unroll
          for (int j = 0; j < 8; ++j) c[i][j] = __fmul_rn(c[i][j], inv_t);  // never fused into what follows
          f(c[i], e, min(8, v - e));
        }
      }
    }
  };

  // ---- pass 1: logsumexp and the thread's greatest s; NaN counts as -inf here as everywhere
  float m = -INFINITY, sm = 0.f, tm = -INFINITY;
  sweep([&](const float (&f)[8], int, int nv) {
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = (j < nv && f[j] == f[j]) ? f[j] : -INFINITY;
    float cm = fmaxf(g[0], g[1]);
#pragma unroll
    for (int j = 2; j < 8; ++j) cm = fmaxf(cm, g[j]);
    tm = fmaxf(tm, cm);
    if (cm > m) {
      sm *= __expf(m - cm);
      m = cm;
    }
    if (m > -INFINITY) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm += __expf(g[j] - m);
    }
  });
  const float wm = wave_max_dpp(m);
  const float ws = wave_sum_dpp(m > -INFINITY ? sm * __expf(m - wm) : 0.f);
  if (lane == 0) {
    redm[wid] = wm;
    reds[wid] = ws;
  }
  tmax[tid] = tm;
  __syncthreads();
  if (tid == 0) {
    float mx = redm[0];
#pragma unroll
    for (int w = 1; w < W; ++w) mx = fmaxf(mx, redm[w]);
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) sum += redm[w] > -INFINITY ? reds[w] * __expf(redm[w] - mx) : 0.f;
    row_lse[row] = mx + __logf(sum);
    row_stat[0] = mx;
    row_stat[1] = sum;
    ctl[0] = 0;
    ctl64[1] = 0;
  }
  __syncthreads();
  const float mx = row_stat[0];
  if (!(mx > -INFINITY)) {  // no finite column: nothing to draw from
    if (tid == 0) {
      ids[row] = -1;
      row_floor[row] = INFINITY;
      row_kept[row] = 0;
    }
    return;
  }
  const bool use_k = top_k >= 1 && top_k < v, use_p = top_p < 1.0;
  auto p_target = [&](u64 z) {  // top_p of the mass z, at least one unit so that the maximum's class stays
    const u64 t = static_cast<u64>(top_p * static_cast<double>(z));
    return t > 0 ? t : u64{1};
  };
  u64 target_p = 0;

  // ---- the bound L: nothing below it survives
  float keep_tm = -INFINITY;
  if (use_k) {
    // the k-th greatest thread maximum: at least k columns are not below it
    int above_me = 0;
    for (int j = 0; j < T; j += 4) {
      const float4 o = *reinterpret_cast<const float4*>(&tmax[j]);
      above_me += (o.x > tm ? 1 : 0) + (o.y > tm ? 1 : 0) + (o.z > tm ? 1 : 0) + (o.w > tm ? 1 : 0);
    }
    keep_tm = above_me < top_k ? -tm : -INFINITY;  // negated: the least such maximum through a max reduction
  } else if (use_p) {
    // the greatest thread maximum at and above which the maxima alone hold the target: a column below it has
    // at least that much mass above it and is removed by the same integer rule the select applies
    target_p = p_target(static_cast<u64>(static_cast<double>(row_stat[1]) * 4294967296.0));
    tq[tid] = tm > -INFINITY ? samp_mass(tm, mx) : 0;
    __syncthreads();
    u64 acc = 0;
    for (int j = 0; j < T; ++j) acc += tmax[j] >= tm ? tq[j] : 0;
    keep_tm = (tm > -INFINITY && acc >= target_p) ? tm : -INFINITY;
  }
  const float wk = wave_max_dpp(keep_tm);
  if (lane == 0) redb[wid] = wk;
  __syncthreads();
  float bound = redb[0];
#pragma unroll
  for (int w = 1; w < W; ++w) bound = fmaxf(bound, redb[w]);
  if (use_k) bound = -bound;  // +inf (no thread qualified) cannot happen: the greatest maximum has nothing above
  if (!use_k && !use_p) bound = -INFINITY;
  const float L = bound;
  auto in_play = [&](float s) { return s >= L && s > -INFINITY; };  // false for NaN

  // ---- stage the columns in play
  int n_cand = kSampCap + 1;
  if (L > -INFINITY || v <= kSampCap) {
    sweep([&](const float (&c)[8], int e, int nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nv && in_play(c[j])) {
          const int slot = atomicAdd(&ctl[0], 1);
          if (slot < kSampCap) {
            cand_s[slot] = c[j];
            cand_c[slot] = e + j;
          }
        }
    });
    __syncthreads();
    n_cand = ctl[0];
  }
  const bool in_lds = n_cand <= kSampCap;
  // f(s, column) for every column in play, from the list or from the row
  auto for_each = [&](auto&& f) {
    if (in_lds) {
      for (int i = tid; i < n_cand; i += T) f(cand_s[i], cand_c[i]);
    } else {
      sweep([&](const float (&c)[8], int e, int nv) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nv && in_play(c[j])) f(c[j], e + j);
      });
    }
  };

  // ---- radix select among the keys >= min_key: the key class c with weight(> c) < target <= weight(>= c);
  // 0 (everything survives) when the whole weight is below the target
  const int low_shift = inv_t == 1.0f ? 32 - SampKey<DT>::bits : 0;
  auto select = [&](bool by_mass, u64 target, uint32_t min_key) -> uint32_t {
    uint32_t mask = 0, val = 0;
#pragma unroll 1
    for (int shift = 24; shift >= low_shift; shift -= 8) {
      if (tid < kSampBins) hist[tid] = 0;
      if (tid == 0) ctl[1] = -1;
      __syncthreads();
      for_each([&](float s, int) {
        const uint32_t k32 = samp_key(s);
        if (k32 >= min_key && (k32 & mask) == val)
          atomicAdd(&hist[(k32 >> shift) & 0xffu], by_mass ? samp_mass(s, mx) : u64{1});
      });
      __syncthreads();
      u64 own = 0, incl = 0;
      if (tid < kSampBins) {  // waves 0..3: inclusive suffix sums inside the wave, then the wave totals
        own = incl = hist[tid];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const u64 o = __shfl_down(incl, off, 64);
          if (lane + off < 64) incl += o;
        }
        if (lane == 0) wtot[wid] = incl;
      }
      __syncthreads();
      if (tid < kSampBins) {
        u64 above = incl - own;
        for (int w = wid + 1; w < kSampBins / 64; ++w) above += wtot[w];
        if (above < target && target <= above + own) {  // at most one bucket
          ctl[1] = tid;
          ctl64[0] = target - above;
        }
      }
      __syncthreads();
      const int b = ctl[1];
      if (b < 0) return 0u;  // block-uniform
      target = ctl64[0];
      val |= static_cast<uint32_t>(b) << shift;
      mask |= 0xffu << shift;
      __syncthreads();
    }
    return val;
  };

  uint32_t floor_key = 0;
  if (use_k) floor_key = select(false, static_cast<u64>(top_k), 0u);
  if (use_p) {
    if (use_k) {  // the survivors' mass; integer, so the order of the additions does not matter
      u64 z = 0;
      for_each([&](float s, int) { z += samp_key(s) >= floor_key ? samp_mass(s, mx) : 0; });
      if (z) atomicAdd(&ctl64[1], z);
      __syncthreads();
      target_p = p_target(ctl64[1]);
    }
    floor_key = select(true, target_p, floor_key);
  }

  // ---- draw among the survivors
  const uint32_t rowterm = samp_rowterm(static_cast<uint32_t>(row));
  float best = -INFINITY, least = INFINITY;
  int best_c = INT_MAX, cnt = 0;
  for_each([&](float s, int col) {
    if (samp_key(s) < floor_key) return;
    const float sc = s + samp_gumbel(static_cast<uint32_t>(col), key, rowterm);
    if (sc > best || (sc == best && col < best_c)) {
      best = sc;
      best_c = col;
    }
    least = fminf(least, s);
    ++cnt;
  });
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64), ol = __shfl_xor(least, off, 64);
    const int oc = __shfl_xor(best_c, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
    if (ob > best || (ob == best && oc < best_c)) {
      best = ob;
      best_c = oc;
    }
    least = fminf(least, ol);
  }
  if (lane == 0) {
    redm[wid] = best;
    redf[wid] = least;
    redc[wid] = best_c;
    redn[wid] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < W; ++w) {
      if (redm[w] > best || (redm[w] == best && redc[w] < best_c)) {
        best = redm[w];
        best_c = redc[w];
      }
      least = fminf(least, redf[w]);
      cnt += redn[w];
    }
    ids[row] = cnt > 0 && best_c < v ? best_c : -1;
    row_floor[row] = least;
    row_kept[row] = cnt;
  }
}

// v <= vp, vp % 8 == 0, 0 < top_p <= 1, top_k >= 0 are checked by the binding as well
hipError_t launch_lm_sample(int dt, const void* logits, int64_t n, int64_t vp, int v, float inv_t, int top_k,
                            double top_p, uint32_t key, int* ids, float* lse, float* floor, int* kept,
                            hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(logits) % 16 != 0 || vp % 8 != 0 || v <= 0 || v > vp || n > INT_MAX || top_k < 0 ||
      !(top_p > 0.0 && top_p <= 1.0) || !(inv_t > 0.f) || vp > (int64_t{1} << 30))
    return hipErrorInvalidValue;
#define LM_SAMPLE(DT)                                                                                     \
  hipLaunchKernelGGL((lm_sample_kernel<DT>), dim3(n), dim3(kSampThreads), 0, st,                          \
                     static_cast<const typename Elem<DT>::S*>(logits), vp, v, inv_t, top_k, top_p, key, ids, lse, \
                     floor, kept)
  switch (dt) {
    case kF32: LM_SAMPLE(kF32); break;
    case kBF16: LM_SAMPLE(kBF16); break;
    case kF16: LM_SAMPLE(kF16); break;
    default: return hipErrorInvalidValue;
  }
#undef LM_SAMPLE
  return hipGetLastError();
}

}  // namespace dlion

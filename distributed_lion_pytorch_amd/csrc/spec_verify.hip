// Speculative sampling's verify step (gfx950): the accept test of every draft token, the residual draw at a
// rejection and the fold to (accepted drafts, next token) per batch row, in one launch over the two read-only logit
// blocks.  Forward only; nothing is written to the logits.
//
// Verify row r = b kk + i has the target row P = t_logits[b, i], the draft row Q = d_logits[b, i], the draft
// token x = drafts[b, i] and the floors lm_sample left on the two rows:
//   sp_j = fp32(P_j) * inv_t, sq_j likewise (one rounded multiply: bit-equal to the values the floors came from)
//   column j survives in p iff sp_j is finite and sp_j >= t_floor[b, i]; in q iff sq_j is finite and >= d_floor[b, i]
//   p_j = exp(sp_j - Mp) / Zp over the p survivors, 0 elsewhere; q_j likewise
//   u = (n + 0.5) 2^-24, n = mix32(mix32(0xFFFFFFFF ^ key) + r * 0x9E3779B1 + 0x85EBCA6B) >> 8
//   accept iff 0 <= x < v and u q_x < p_x (the product in fp64 on the fp32 p_x and q_x: exact)
//   rejected: resid = argmax_j log(p_j - q_j) + g_j over the columns with p_j > q_j, g_j lm_sample's Gumbel noise of
//   (j, key, r), the lowest column on ties; no such column: argmax over the p survivors of sp_j + g_j; none: -1
//   accepted[b] = the leading accepted drafts of row b; next[b] = bonus[b] if all kk, else resid[b, accepted[b]]
//
// One 512-thread block per (i, b).
//   sweep 1   both rows together, 16-byte loads, kSpecUnroll chunks of 8 per row in flight; two online (max, sum of
//             exp) pairs over the survivors with the accurate expf, chunks without a survivor skipped; DPP wave
//             reductions, then the 8 waves through LDS in wave order (no float atomics: equal inputs, equal bits).
//   accept    thread 0 reads P_x and Q_x, forms p_x, q_x and the flag; the flag is block-uniform through LDS.
//   sweep 2   rejected rows only: both rows again (L2), w_j = p_j - q_j with the reciprocals of Zp and Zq, the
//             Gumbel score where w_j > 0, (score, column) reduced by max / lowest column as lm_sample's draw is.
//             A second turn of the same loop is the fallback on sp_j + g_j.
//   fold      thread 0 writes the row's outputs, fences, and bumps arrive[b]; the block that finds kk - 1 there
//             reads the kk flags and tokens of row b (device-scope loads), writes accepted[b] and next[b] and sets
//             arrive[b] back to 0.  No block waits for another.
#include "sampling.h"

#include <climits>

namespace dlion {

constexpr int kSpecThreads = 512;
constexpr int kSpecUnroll = 4;  // chunks of 8 logits in flight per thread and row
constexpr int kSpecMaxDrafts = 7;

__device__ __forceinline__ bool spec_alive(float s, float floor) {  // false for NaN and both infinities
  return s >= floor && fabsf(s) < INFINITY;
}

// one chunk of 8 into an online (max, sum of exp(s - max)) pair; g holds -inf where the column takes no part
__device__ __forceinline__ void spec_online(const float (&g)[8], float& m, float& sm) {
  float cm = fmaxf(g[0], g[1]);
#pragma unroll
  for (int j = 2; j < 8; ++j) cm = fmaxf(cm, g[j]);
  if (!(cm > -INFINITY)) return;
  if (cm > m) {
    sm *= expf(m - cm);
    m = cm;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sm += expf(g[j] - m);
}

template <int DT>
__global__ void __launch_bounds__(kSpecThreads)
spec_verify_kernel(const typename Elem<DT>::S* __restrict__ t_logits, const typename Elem<DT>::S* __restrict__ d_logits,
                   const int* __restrict__ drafts, const float* __restrict__ t_floor,
                   const float* __restrict__ d_floor, const int* __restrict__ bonus, int kk, int64_t vp, int v,
                   float inv_t, uint32_t key, int* arrive, int* flags, int* resid, float* __restrict__ px_out,
                   float* __restrict__ qx_out, int* __restrict__ accepted, int* __restrict__ next) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int T = kSpecThreads, W = kSpecThreads / 64, U = kSpecUnroll;
  __shared__ float red_mp[W], red_sp[W], red_mq[W], red_sq[W], red_b[W];
  __shared__ int red_c[W];
  __shared__ float stat[4];  // Mp, Zp, Mq, Zq
  __shared__ int ctl[2];     // the flag, the residual token
  const int i = blockIdx.x, b = blockIdx.y;
  const int r = b * kk + i;
  const S* P = t_logits + (static_cast<int64_t>(b) * (kk + 1) + i) * vp;
  const S* Q = d_logits + static_cast<int64_t>(r) * vp;
  const float tf = t_floor[b * (kk + 1) + i], df = d_floor[r];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

  // f(sp[8], sq[8], first column, real columns in the chunk); columns at and past v take part in nothing
  auto sweep = [&](auto&& f) {
    for (int base = tid * 8; base < v; base += T * 8 * U) {
      float cp[U][8], cq[U][8];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int e = base + k * T * 8;
        if (e < v) {  // v <= vp and vp % 8 == 0 keep every chunk inside its row
          E::load8(P + e, cp[k]);
          E::load8(Q + e, cq[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int e = base + k * T * 8;
        if (e < v) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            cp[k][j] = __fmul_rn(cp[k][j], inv_t);  // never fused into what follows
            cq[k][j] = __fmul_rn(cq[k][j], inv_t);
          }
          f(cp[k], cq[k], e, min(8, v - e));
        }
      }
    }
  };

  // ---- sweep 1: (max, sum of exp) of the survivors of both rows
  float mp = -INFINITY, zp = 0.f, mq = -INFINITY, zq = 0.f;
  sweep([&](const float (&sp)[8], const float (&sq)[8], int, int nv) {
    float gp[8], gq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      gp[j] = (j < nv && spec_alive(sp[j], tf)) ? sp[j] : -INFINITY;
      gq[j] = (j < nv && spec_alive(sq[j], df)) ? sq[j] : -INFINITY;
    }
    spec_online(gp, mp, zp);
    spec_online(gq, mq, zq);
  });
  const float wmp = wave_max_dpp(mp), wmq = wave_max_dpp(mq);
  const float wzp = wave_sum_dpp(mp > -INFINITY ? zp * expf(mp - wmp) : 0.f);
  const float wzq = wave_sum_dpp(mq > -INFINITY ? zq * expf(mq - wmq) : 0.f);
  if (lane == 0) {
    red_mp[wid] = wmp;
    red_sp[wid] = wzp;
    red_mq[wid] = wmq;
    red_sq[wid] = wzq;
  }
  __syncthreads();

  // ---- the accept test
  const uint32_t rowterm = samp_rowterm(static_cast<uint32_t>(r));
  if (tid == 0) {
    float Mp = red_mp[0], Mq = red_mq[0];
#pragma unroll
    for (int w = 1; w < W; ++w) {
      Mp = fmaxf(Mp, red_mp[w]);
      Mq = fmaxf(Mq, red_mq[w]);
    }
    float Zp = 0.f, Zq = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      Zp += red_mp[w] > -INFINITY ? red_sp[w] * expf(red_mp[w] - Mp) : 0.f;
      Zq += red_mq[w] > -INFINITY ? red_sq[w] * expf(red_mq[w] - Mq) : 0.f;
    }
    const int x = drafts[r];
    float px = 0.f, qx = 0.f;
    bool ok = false;
    if (x >= 0 && x < v) {  // the rows are read at x only inside [0, v)
      const float spx = __fmul_rn(E::to_f(P[x]), inv_t), sqx = __fmul_rn(E::to_f(Q[x]), inv_t);
      if (spec_alive(spx, tf)) px = __fdiv_rn(expf(spx - Mp), Zp);
      if (spec_alive(sqx, df)) qx = __fdiv_rn(expf(sqx - Mq), Zq);
      ok = samp_uniform(key, rowterm) * static_cast<double>(qx) < static_cast<double>(px);
    }
    px_out[r] = px;
    qx_out[r] = qx;
    stat[0] = Mp;
    stat[1] = Zp;
    stat[2] = Mq;
    stat[3] = Zq;
    ctl[0] = ok ? 1 : 0;
    ctl[1] = -1;
  }
  __syncthreads();

  // ---- sweep 2, rejected rows only (block-uniform): the residual draw, then its fallback
  if (ctl[0] == 0) {
    const float Mp = stat[0], Mq = stat[2];
    const float rzp = __frcp_rn(stat[1]), rzq = __frcp_rn(stat[3]);
#pragma unroll 1
    for (int turn = 0; turn < 2; ++turn) {
      float best = -INFINITY;
      int best_c = INT_MAX;
      sweep([&](const float (&sp)[8], const float (&sq)[8], int e, int nv) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool ap = j < nv && spec_alive(sp[j], tf);
          float base_score = -INFINITY;
          if (turn == 0) {
            const float pj = ap ? __fmul_rn(expf(sp[j] - Mp), rzp) : 0.f;
            const float qj = (j < nv && spec_alive(sq[j], df)) ? __fmul_rn(expf(sq[j] - Mq), rzq) : 0.f;
            const float w = pj - qj;
            if (w > 0.f) base_score = logf(w);
          } else if (ap) {
            base_score = sp[j];
          }
          if (base_score > -INFINITY) {
            const float sc = base_score + samp_gumbel(static_cast<uint32_t>(e + j), key, rowterm);
            if (sc > best || (sc == best && e + j < best_c)) {
              best = sc;
              best_c = e + j;
            }
          }
        }
      });
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oc = __shfl_xor(best_c, off, 64);
        if (ob > best || (ob == best && oc < best_c)) {
          best = ob;
          best_c = oc;
        }
      }
      if (lane == 0) {
        red_b[wid] = best;
        red_c[wid] = best_c;
      }
      __syncthreads();
      if (tid == 0) {
#pragma unroll
        for (int w = 1; w < W; ++w)
          if (red_b[w] > best || (red_b[w] == best && red_c[w] < best_c)) {
            best = red_b[w];
            best_c = red_c[w];
          }
        ctl[1] = best_c < v ? best_c : -1;
      }
      __syncthreads();
      if (ctl[1] >= 0) break;  // block-uniform
    }
  }

  // ---- the row's outputs and the fold by the last block of batch row b to arrive
  if (tid == 0) {
    flags[r] = ctl[0];
    resid[r] = ctl[1];
    __threadfence();
    if (atomicAdd(&arrive[b], 1) == kk - 1) {
      __threadfence();
      int a = 0;
      while (a < kk && __hip_atomic_load(&flags[b * kk + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ++a;
      accepted[b] = a;
      next[b] = a == kk ? bonus[b] : __hip_atomic_load(&resid[b * kk + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      arrive[b] = 0;  // ready for the next launch
    }
  }
}

// shapes: t_logits [batch, kk + 1, vp], d_logits [batch, kk, vp]; checked by the binding as well
hipError_t launch_spec_verify(int dt, const void* t_logits, const void* d_logits, const int* drafts,
                              const float* t_floor, const float* d_floor, const int* bonus, int64_t batch, int kk,
                              int64_t vp, int v, float inv_t, uint32_t key, int* arrive, int* flags, int* resid,
                              float* px, float* qx, int* accepted, int* next, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(t_logits) % 16 != 0 || reinterpret_cast<uintptr_t>(d_logits) % 16 != 0 ||
      vp % 8 != 0 || v <= 0 || v > vp || vp > (int64_t{1} << 30) || kk < 1 || kk > kSpecMaxDrafts || batch < 0 ||
      batch > 65535 || !(inv_t > 0.f))
    return hipErrorInvalidValue;
#define SPEC_VERIFY(DT)                                                                                         \
  hipLaunchKernelGGL((spec_verify_kernel<DT>), dim3(kk, batch), dim3(kSpecThreads), 0, st,                      \
                     static_cast<const typename Elem<DT>::S*>(t_logits),                                        \
                     static_cast<const typename Elem<DT>::S*>(d_logits), drafts, t_floor, d_floor, bonus, kk, vp, v, \
                     inv_t, key, arrive, flags, resid, px, qx, accepted, next)
  switch (dt) {
    case kF32: SPEC_VERIFY(kF32); break;
    case kBF16: SPEC_VERIFY(kBF16); break;
    case kF16: SPEC_VERIFY(kF16); break;
    default: return hipErrorInvalidValue;
  }
#undef SPEC_VERIFY
  return hipGetLastError();
}

}  // namespace dlion

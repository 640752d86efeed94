// Per-head q/k RMSNorm fused with the rotary embedding (Qwen3), forward and backward.
//
// For a head row x of D bf16 elements (D = 64 or 128):
//   r = rsqrt(mean(x^2) + eps),  xh = x r,  y = xh gamma,  z = rope(y)
// with the rotate-half convention and the [>= T, D] bf16 tables of rope_kernel
// (elementwise_kernels.hip; table row t = token row % T).  Heads [0, split) of a
// token take gamma_a, heads [split, Hx) gamma_b: q | k of the fused projection
// output are normalised and rotated by one launch.
//
// Mapping.  The op is memory-bound, so every lane moves 16 bytes (8 bf16,
// cdna_hip_programming.md Guideline 13): a head row is D / 8 = 16 (or 8)
// adjacent lanes, 4 (or 8) head rows per wave.  The row sums are a butterfly of
// DPP moves inside those lanes (quad_perm, quad_perm, row_half_mirror,
// row_mirror): every lane of the row adds the same two operands at every step,
// so all of them hold bit-identical sums.  The rotate-half partner of a lane's
// 8 dims sits D / 16 lanes away and comes by DPP as well (row_ror:8 for 16
// lanes, row_half_mirror + a quad reversal for 8).  No LDS, no atomics.
//
// Every loop has a block-uniform trip count and rows past the end are clamped
// (read again, never stored), so the lanes a DPP move reads are always active.
#include "common.h"
#include "kernels.h"
#include "rope_norm.h"

// No implicit FMA contraction in this file: the arithmetic of a head row must not depend on which unrolled
// slot of the backward's head loop it lands in (the compiler is free to fuse different products in each), or
// q | k in one launch and q, k in launches of their own differ in the last bit.  Fused multiply-adds are
// written out where they are wanted.
#pragma clang fp contract(off)

namespace dlion {
namespace {

using E = Elem<kBF16>;

__device__ __forceinline__ void store8f(float* p, const float (&o)[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(o[4], o[5], o[6], o[7]);
}

template <int D>
__global__ void __launch_bounds__(256) qk_norm_rope_fwd_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ ga, const uint16_t* __restrict__ gb,
    const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn, uint16_t* __restrict__ y,
    float* __restrict__ rstd, int64_t n_hr, int T, int Hx, int split, float eps, int64_t x_ld) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES;
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int d0 = sub * 8;
  const bool first = sub < LANES / 2;
  float wa[8], wb[8];
  E::load8(ga + d0, wa);
  E::load8(gb + d0, wb);
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * GROUPS; base < n_hr;
       base += static_cast<int64_t>(gridDim.x) * GROUPS) {
    const int64_t hr = base + grp;  // token row * Hx + head
    const bool valid = hr < n_hr;
    const int64_t hrc = valid ? hr : n_hr - 1;
    const int64_t row = hrc / Hx;
    const int h = static_cast<int>(hrc - row * Hx);
    const int64_t tb = (row % T) * D + d0;
    float v[8], c[8], s[8], w[8], o[8];
    E::load8(x + row * x_ld + static_cast<int64_t>(h) * D + d0, v);
    E::load8(cs + tb, c);
    E::load8(sn + tb, s);
    const bool a = h < split;
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = a ? wa[j] : wb[j];
    const float r = qk_norm_rope_row<LANES>(v, w, c, s, eps, first, o);  // rope_norm.h, shared with decode.hip
    if (valid) {
      E::store8(y + hr * D + d0, o);
      if (sub == 0) rstd[hr] = r;
    }
  }
}

// In place on g (token stride g_ld).  A part is one head-row lane group: it owns
// the token rows [p rpp, min((p + 1) rpp, rows)) and leaves its own fp32 sums
// part[p][0][:] (heads < split) and part[p][1][:] (the rest).  U head rows are
// loaded before the first of them is stored: g is read and written through one
// pointer, which keeps the compiler from moving the loads up itself.
template <int D, bool ROT>
__global__ void __launch_bounds__(256) qk_norm_rope_bwd_kernel(
    uint16_t* g, const uint16_t* __restrict__ x, const float* __restrict__ rstd, const uint16_t* __restrict__ ga,
    const uint16_t* __restrict__ gb, const uint16_t* __restrict__ cs, const uint16_t* __restrict__ sn,
    float* __restrict__ part, int parts, int64_t rows, int64_t rpp, int T, int Hx, int split, int64_t g_ld,
    int64_t x_ld) {
  constexpr int LANES = D / 8, GROUPS = 256 / LANES, U = 4;
  const int sub = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int d0 = sub * 8;
  const bool first = sub < LANES / 2;
  const int64_t p = static_cast<int64_t>(blockIdx.x) * GROUPS + grp;
  const bool live = p < parts;
  const int64_t r0 = live ? min(p * rpp, rows) : rows;
  const int64_t r1 = min(r0 + rpp, rows);
  float wa[8], wb[8], acc_a[8], acc_b[8];
  E::load8(ga + d0, wa);
  E::load8(gb + d0, wb);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc_a[j] = acc_b[j] = 0.f;
  for (int64_t i = 0; i < rpp; ++i) {
    const bool rvalid = r0 + i < r1;
    const int64_t row = rvalid ? r0 + i : rows - 1;
    const int64_t tb = (row % T) * D + d0;
    float c[8], s[8];
    if (ROT) {
      E::load8(cs + tb, c);
      E::load8(sn + tb, s);
    }
    uint16_t* grow = g + row * g_ld + d0;
    const uint16_t* xrow = x + row * x_ld + d0;
    const float* rrow = rstd + row * Hx;
    for (int h0 = 0; h0 < Hx; h0 += U) {
      uint4 graw[U], xraw[U];
      float rs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int h = min(h0 + u, Hx - 1);
        graw[u] = *reinterpret_cast<const uint4*>(grow + static_cast<int64_t>(h) * D);
        xraw[u] = *reinterpret_cast<const uint4*>(xrow + static_cast<int64_t>(h) * D);
        rs[u] = rrow[h];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int h = h0 + u;
        const bool valid = rvalid && h < Hx;
        const bool a = h < split;
        const uint32_t gw[4] = {graw[u].x, graw[u].y, graw[u].z, graw[u].w};
        const uint32_t xw[4] = {xraw[u].x, xraw[u].y, xraw[u].z, xraw[u].w};
        float dy[8], xh[8], gg[8], dx[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dy[2 * j] = bf16_to_f32(static_cast<uint16_t>(gw[j] & 0xffffu));
          dy[2 * j + 1] = bf16_to_f32(static_cast<uint16_t>(gw[j] >> 16));
          xh[2 * j] = bf16_to_f32(static_cast<uint16_t>(xw[j] & 0xffffu)) * rs[u];
          xh[2 * j + 1] = bf16_to_f32(static_cast<uint16_t>(xw[j] >> 16)) * rs[u];
        }
        if (ROT) {  // g holds dz: the transpose rotation first
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float pz = partner<LANES>(dy[j] * s[j]);
            dy[j] = dy[j] * c[j] + (first ? pz : -pz);
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) gg[j] = dy[j] * (a ? wa[j] : wb[j]);
        const float m = head_sum<LANES>(dot8(gg, xh)) * (1.f / D);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          dx[j] = rs[u] * (gg[j] - xh[j] * m);
          const float term = dy[j] * xh[j];
          acc_a[j] += (valid && a) ? term : 0.f;
          acc_b[j] += (valid && !a) ? term : 0.f;
        }
        if (valid) E::store8(grow + static_cast<int64_t>(h) * D, dx);
      }
    }
  }
  if (live) {
    store8f(part + (p * 2) * D + d0, acc_a);
    store8f(part + (p * 2 + 1) * D + d0, acc_b);
  }
}

}  // namespace

hipError_t launch_qk_norm_rope_fwd(const void* x, const void* gamma_a, const void* gamma_b, const void* cos,
                                   const void* sin, void* y, float* rstd, int64_t rows, int T, int Hx, int D,
                                   int split, float eps, int64_t x_ld, hipStream_t st) {
  const int64_t n_hr = rows * Hx;
  if (n_hr == 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  const int groups = 256 / (D / 8);
  const int64_t blocks = (n_hr + groups - 1) / groups;
  const dim3 grid(static_cast<unsigned>(blocks < (1 << 20) ? blocks : (1 << 20)));
  auto* X = static_cast<const uint16_t*>(x);
  auto* A = static_cast<const uint16_t*>(gamma_a);
  auto* Bg = static_cast<const uint16_t*>(gamma_b);
  auto* C = static_cast<const uint16_t*>(cos);
  auto* S = static_cast<const uint16_t*>(sin);
  auto* Y = static_cast<uint16_t*>(y);
  if (D == 128)
    hipLaunchKernelGGL(qk_norm_rope_fwd_kernel<128>, grid, dim3(256), 0, st, X, A, Bg, C, S, Y, rstd, n_hr, T, Hx, split,
                       eps, x_ld);
  else
    hipLaunchKernelGGL(qk_norm_rope_fwd_kernel<64>, grid, dim3(256), 0, st, X, A, Bg, C, S, Y, rstd, n_hr, T, Hx, split,
                       eps, x_ld);
  return hipGetLastError();
}

hipError_t launch_qk_norm_rope_bwd(void* g, const void* x, const float* rstd, const void* gamma_a, const void* gamma_b,
                                   const void* cos, const void* sin, float* part, int parts, int64_t rows, int T,
                                   int Hx, int D, int split, int64_t g_ld, int64_t x_ld, hipStream_t st) {
  if (parts <= 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  if (rows * Hx == 0) return hipMemsetAsync(part, 0, sizeof(float) * parts * 2 * D, st);
  const int groups = 256 / (D / 8);
  const dim3 grid(static_cast<unsigned>((parts + groups - 1) / groups));
  const int64_t rpp = (rows + parts - 1) / parts;
  auto* G = static_cast<uint16_t*>(g);
  auto* X = static_cast<const uint16_t*>(x);
  auto* A = static_cast<const uint16_t*>(gamma_a);
  auto* Bg = static_cast<const uint16_t*>(gamma_b);
  auto* C = static_cast<const uint16_t*>(cos);
  auto* S = static_cast<const uint16_t*>(sin);
#define DLION_QK_BWD(DD, ROT)                                                                                        \
  hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<DD, ROT>), grid, dim3(256), 0, st, G, X, rstd, A, Bg, C, S, part, parts, \
                     rows, rpp, T, Hx, split, g_ld, x_ld)
  if (D == 128) {
    if (cos != nullptr) DLION_QK_BWD(128, true); else DLION_QK_BWD(128, false);
  } else {
    if (cos != nullptr) DLION_QK_BWD(64, true); else DLION_QK_BWD(64, false);
  }
#undef DLION_QK_BWD
  return hipGetLastError();
}

}  // namespace dlion

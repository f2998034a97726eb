// Device primitives shared by the kernel files: the f64 MFMA, 64-bit lane
// moves, the wave-level sync, the Newton reciprocal, and the block sums.
// gfx950 (CDNA4) only; wave = 64 lanes.
#pragma once

#include "dopt_internal.h"

namespace dopt {

typedef double d4 __attribute__((ext_vector_type(4)));

// D = A·B + C, 16×16×4 f64: one f64 of A and of B per lane, four results
// (C/D: col = lane & 15, row = (lane >> 4) + 4·reg)
__device__ __forceinline__ d4 mfma_f64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// a double through one DPP lane move (VALU, no LDS crossbar), as two 32-bit
// halves; lanes the move does not write keep v, or get 0 with ZERO
template <int CTRL, int ROWMASK, bool ZERO = false>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(ZERO ? 0 : (int)b, (int)b, CTRL, ROWMASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(ZERO ? 0 : (int)(b >> 32), (int)(b >> 32), CTRL, ROWMASK, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// lane l's x (l wave-uniform): two v_readlane_b32 into an SGPR pair
__device__ __forceinline__ double readlane_d(double x, int l) {
  const unsigned long long v = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// 1/d: v_rcp_f64 + two Newton steps
__device__ __forceinline__ double rcp_nr(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  return fma(fma(-d, r, 1.0), r, r);
}

// one wave's LDS writes visible to its own later reads, no workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- wave sums --------------------------------------------------------------
// xor butterfly (32, 16, … 1) through __shfl_xor; the sum in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// by DPP: quad xor 1 / 2, the half-row and row mirrors, then row_bcast:15 / 31
// carry the rows' totals up; the full sum lands in lane 63 (the other lanes
// hold partial sums)
__device__ __forceinline__ double wave_sum63(double v) {
  v += dpp_f64<0xB1, 0xF>(v);          // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E, 0xF>(v);          // quad_perm [2,3,0,1]
  v += dpp_f64<0x141, 0xF>(v);         // row_half_mirror
  v += dpp_f64<0x140, 0xF>(v);         // row_mirror
  v += dpp_f64<0x142, 0xA, true>(v);   // row_bcast:15 → rows 1, 3
  v += dpp_f64<0x143, 0xC, true>(v);   // row_bcast:31 → rows 2, 3
  return v;
}
// the DPP sum in every lane: broadcast from lane 63
__device__ __forceinline__ double cwave_sum(double v) { return readlane_d(wave_sum63(v), 63); }

// The per-lane partial sums of a dense column sweep by one wave,
//   for (i = lane; i < rows; i += 64) acc = fma(col[i], w[i], acc),
// from the column's sparse entries k0 ≤ k < k1 (rows ri ascending, values cv):
// lane L adds the entries with ri % 64 == L in ascending order, so each lane
// ends with the dense sweep's bits (an absent entry is a zero there, and
// fma(0, w, acc) == acc for finite w).  The wave walks the entries 64 at a
// time (coalesced loads) and hands each to its lane by broadcast.  Called by
// all 64 lanes with wave-uniform k0, k1.
__device__ __forceinline__ double sparse_col_lane_sum(const int32_t* __restrict__ ri, const double* __restrict__ cv,
                                                      int64_t k0, int64_t k1, const double* __restrict__ w,
                                                      double acc) {
  const int lane = threadIdx.x & 63;
  for (int64_t c = k0; c < k1; c += 64) {
    const int64_t k = c + lane;
    const bool in = k < k1;
    const int i = in ? ri[k] : 0;
    const double a = in ? cv[k] : 0.0;
    const double wi = in ? w[i] : 0.0;
    const int cnt = k1 - c < 64 ? (int)(k1 - c) : 64;
    for (int t = 0; t < cnt; ++t) {
      const int it = __shfl(i, t);
      const double at = __shfl(a, t), wt = __shfl(wi, t);
      if ((it & 63) == lane) acc = fma(at, wt, acc);
    }
  }
  return acc;
}

// ---- block sums -------------------------------------------------------------
// Every thread gets the result; `red` = LDS scratch of one double per wave.
// They differ in summation order, so each kernel keeps the one it was
// validated with: results change in the last bits otherwise.
//
// 4 waves: xor-butterfly wave sums, then ((w0 + w1) + w2) + w3
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double r = red[0] + red[1] + red[2] + red[3];
  return r;
}

// 16 waves: xor-butterfly wave sums, then 0 + w0 + w1 + … + w15 in order
__device__ __forceinline__ double sp_block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) r += red[w];
  return r;
}

// 4 waves: DPP wave sums, then ((w0 + w1) + w2) + w3
__device__ __forceinline__ double cblock_sum(double v, double* red) {
  v = cwave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// 16 waves: DPP wave sums, then 0 + w0 + w1 + … + w15 in order
__device__ __forceinline__ double vblock_sum(double v, double* red) {
  v = cwave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += red[k];
  return s;
}

// after a kernel launch: throws on a launch error
inline void check_launch() { DOPT_CHECK_HIP(hipGetLastError()); }

}  // namespace dopt

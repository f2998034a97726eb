// IterativeSolvers.lsqr (0.9 defaults: damp = 0, atol = btol = √eps, conlim =
// 1/√eps), restated operation for operation — the specification is
// oracle/lsqr.py.  This header owns what one LSQR step computes: the scalar
// state, the plane rotation, the ‖x‖ / cond / ‖r‖ estimates and stopping tests,
// the block-strided vector phases, and the driver of one sequence per
// workgroup.  A kernel owns its operator (A·v, Aᵀ·u), its reduction order (the
// block sum it passes, device_prims.h) and its sequencing (one sequence,
// several in lockstep, or one launch per phase).
//
// Every kernel that includes this computes the same expressions, which is
// what makes co-iterated, multi-seed and split results equal single runs bit
// for bit: change a line here and it changes for all of them.
#pragma once

#include <cstdint>

namespace dopt {

// scalars of one sequence; kernels derive from it for their own flags
struct LsqrScalars {
  double alpha, beta, anorm, ddnorm, xxnorm, zz, sn2, cs2, rhobar, phibar, bnorm;
  double rnorm, arnorm, xnorm;   // terminal estimates, with anorm
  int32_t it, istop;
};

// after the first bidiagonalisation step: α = ‖Aᵀu‖, β = ‖b‖
__device__ __forceinline__ void lsqr_begin(LsqrScalars& st, double alpha, double beta) {
  st.alpha = alpha;
  st.beta = beta;
  st.anorm = st.ddnorm = st.xxnorm = st.zz = st.sn2 = 0.0;
  st.cs2 = -1.0;
  st.rhobar = alpha;
  st.phibar = st.bnorm = beta;
  st.rnorm = st.arnorm = st.xnorm = 0.0;
  st.it = 0;
  st.istop = 0;
}

// ‖A‖_F estimate, once β of this step is known and > 0
__device__ __forceinline__ void lsqr_anorm(LsqrScalars& st, double alpha, double beta) {
  st.anorm = sqrt(st.anorm * st.anorm + alpha * alpha + beta * beta);
}

// One step's plane rotation (lsqr!, the loop body after the
// bidiagonalisation): x += t1·w, w ← v + t2·w follow from it.
struct LsqrStep {
  double rho, theta, rhobar, phi, phibar, tau, t1, t2;
};
__device__ __forceinline__ LsqrStep lsqr_rotate(const LsqrScalars& st, double alpha, double beta) {
  LsqrStep g;
  const double rhobar1 = st.rhobar;
  g.rho = hypot(rhobar1, beta);
  const double cs = rhobar1 / g.rho, sn = beta / g.rho;
  g.theta = sn * alpha;
  g.rhobar = -cs * alpha;
  g.phi = cs * st.phibar;
  g.phibar = sn * st.phibar;
  g.tau = sn * g.phi;
  g.t1 = g.phi / g.rho;
  g.t2 = -g.theta / g.rho;
  return g;
}

// After the x / w update (ddnorm = st.ddnorm + Σw²/ρ²): commits the step to
// st, its estimates and stopping tests; returns istop (0: go on).
__device__ __forceinline__ int lsqr_tests(LsqrScalars& st, const LsqrStep& g, double alpha, double ddnorm,
                                          int maxiter) {
  const double eps = 2.220446049250313e-16;
  const double atol = sqrt(eps), btol = sqrt(eps), ctol = sqrt(eps);
  const double anorm = st.anorm, bnorm = st.bnorm;
  const double delta = st.sn2 * g.rho, gambar = -st.cs2 * g.rho;
  const double rhs_ = g.phi - delta * st.zz;
  const double zbar = rhs_ / gambar;
  const double xnorm = sqrt(st.xxnorm + zbar * zbar);
  const double gamma = hypot(gambar, g.theta);
  st.cs2 = gambar / gamma;
  st.sn2 = g.theta / gamma;
  st.zz = rhs_ / gamma;
  st.xxnorm += st.zz * st.zz;
  const double acond = anorm * sqrt(ddnorm);
  const double rnorm = sqrt(g.phibar * g.phibar);   // damp = 0: res2 == 0.0, and sqrt(φ̄² + 0.0) is the same double
  const double arnorm = alpha * fabs(g.tau);
  const double test1 = rnorm / bnorm;
  const double test2 = (anorm * rnorm != 0.0) ? arnorm / (anorm * rnorm) : 0.0;
  const double test3 = (acond != 0.0) ? 1.0 / acond : 0.0;
  const double t1r = test1 / (1.0 + anorm * xnorm / bnorm);
  const double rtol = btol + atol * anorm * xnorm / bnorm;
  int istop = 0;
  if (st.it >= maxiter) istop = 7;
  if (1.0 + test3 <= 1.0) istop = 6;
  if (1.0 + test2 <= 1.0) istop = 5;
  if (1.0 + t1r <= 1.0) istop = 4;
  if (test3 <= ctol) istop = 3;
  if (test2 <= atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  st.alpha = alpha;
  st.rhobar = g.rhobar;
  st.phibar = g.phibar;
  st.ddnorm = ddnorm;
  st.istop = istop;
  st.rnorm = rnorm;
  st.arnorm = arnorm;
  st.xnorm = xnorm;
  return istop;
}

// ---- vector phases ----------------------------------------------------------
// Thread t of a TPB-thread workgroup takes entries t, t + TPB, …; SUM is the
// kernel's block sum (double v, double* red) → double, `red` its LDS scratch.
// The norms accumulate by explicit fma, the updates are plain products and
// sums.

// u ← b, x ← 0; returns ‖b‖²
template <int TPB, double (*SUM)(double, double*)>
__device__ __forceinline__ double lsqr_load_rhs(const double* rb, double* u, double* x, int N, double* red) {
  double bb = 0.0;
  for (int i = threadIdx.x; i < N; i += TPB) {
    const double r = rb[i];
    u[i] = r;
    x[i] = 0.0;
    bb = fma(r, r, bb);
  }
  return SUM(bb, red);
}

// returns ‖v‖²
template <int TPB, double (*SUM)(double, double*)>
__device__ __forceinline__ double lsqr_norm2(const double* v, int N, double* red) {
  double aa = 0.0;
  for (int i = threadIdx.x; i < N; i += TPB) aa = fma(v[i], v[i], aa);
  return SUM(aa, red);
}

// y ← y / d (no barrier)
template <int TPB>
__device__ __forceinline__ void lsqr_scale(double* y, int N, double d) {
  for (int i = threadIdx.x; i < N; i += TPB) y[i] /= d;
}

// v ← v / α, w ← v (no barrier)
template <int TPB>
__device__ __forceinline__ void lsqr_scale_copy(double* v, double* w, int N, double alpha) {
  for (int i = threadIdx.x; i < N; i += TPB) { v[i] /= alpha; w[i] = v[i]; }
}

// y ← tmp − c·y; returns ‖y‖².  The two bidiagonalisation updates:
// u ← A·v − α·u and v ← Aᵀ·u − β·v.
template <int TPB, double (*SUM)(double, double*)>
__device__ __forceinline__ double lsqr_bidiag(double* y, const double* tmp, double c, int N, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += TPB) { const double yi = tmp[i] - c * y[i]; y[i] = yi; s = fma(yi, yi, s); }
  return SUM(s, red);
}

// x += t1·w, w ← v + t2·w; returns Σw² of the w read
template <int TPB, double (*SUM)(double, double*)>
__device__ __forceinline__ double lsqr_update_xw(double* x, double* w, const double* v, double t1, double t2, int N,
                                                 double* red) {
  double sw = 0.0;
  for (int i = threadIdx.x; i < N; i += TPB) {
    const double wi = w[i];
    sw = fma(wi, wi, sw);
    x[i] = x[i] + t1 * wi;
    w[i] = v[i] + t2 * wi;
  }
  return SUM(sw, red);
}

// the step after both products: rotation, x / w update, tests; returns istop
template <int TPB, double (*SUM)(double, double*)>
__device__ __forceinline__ int lsqr_finish_step(LsqrScalars& st, double* x, double* w, const double* v, int N,
                                                int maxiter, double* red) {
  const LsqrStep g = lsqr_rotate(st, st.alpha, st.beta);
  const double sw = lsqr_update_xw<TPB, SUM>(x, w, v, g.t1, g.t2, N, red);
  return lsqr_tests(st, g, st.alpha, st.ddnorm + sw / (g.rho * g.rho), maxiter);
}

// ---- one sequence per workgroup -----------------------------------------------
// Solves min ‖op·x − b‖ from x = 0.  OP gives mul(v, out): out = A·v and
// tmul(u, out): out = Aᵀ·u, each ending in a workgroup barrier.  b with
// ‖b‖ ≤ rhs_zero_tol, Aᵀb = 0 or maxiter = 0 leave x = 0, istop = 0, it = 0.
// x, u, v, w, tmp: N doubles each.  The caller's barrier comes before it
// reads x.
template <int TPB, double (*SUM)(double, double*), class OP>
__device__ __forceinline__ void lsqr_solve(LsqrScalars& st, const OP& op, const double* rb, double rhs_zero_tol,
                                           int maxiter, double* x, double* u, double* v, double* w, double* tmp,
                                           int N, double* red) {
  st = LsqrScalars{};
  const double beta = sqrt(lsqr_load_rhs<TPB, SUM>(rb, u, x, N, red));
  if (!(beta > rhs_zero_tol)) return;
  lsqr_scale<TPB>(u, N, beta);
  __syncthreads();
  op.tmul(u, v);
  const double alpha = sqrt(lsqr_norm2<TPB, SUM>(v, N, red));
  if (!(alpha > 0.0)) return;
  lsqr_scale_copy<TPB>(v, w, N, alpha);
  __syncthreads();
  lsqr_begin(st, alpha, beta);
  while (st.it < maxiter) {
    ++st.it;
    op.mul(v, tmp);
    st.beta = sqrt(lsqr_bidiag<TPB, SUM>(u, tmp, st.alpha, N, red));
    if (st.beta > 0.0) {
      lsqr_scale<TPB>(u, N, st.beta);
      __syncthreads();
      lsqr_anorm(st, st.alpha, st.beta);
      op.tmul(u, tmp);
      st.alpha = sqrt(lsqr_bidiag<TPB, SUM>(v, tmp, st.beta, N, red));
      if (st.alpha > 0.0) lsqr_scale<TPB>(v, N, st.alpha);
      __syncthreads();
    }
    const int istop = lsqr_finish_step<TPB, SUM>(st, x, w, v, N, maxiter, red);
    __syncthreads();
    if (istop) break;
  }
}

}  // namespace dopt

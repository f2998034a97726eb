// Parameter (ParametricOptInterface) accumulation for the QP and the conic
// back-end, batched (the conic half: "conic parameter accumulation" below):
// the reference's POI glue (src/parameters.jl) turns parameter tangents into
// constraint / objective tangents before forward_differentiate! and folds the
// reverse getters into parameter gradients after reverse_differentiate!.
//
// A parametric term t = (parameter p_t, kind_t, index_t, coefficient c_t):
//   kind 0  parameter term of LessThan row i   (_constraint_*!, ParametricAffineFunction)
//   kind 1  parameter term of EqualTo row i
//   kind 2  parameter term of the objective     (_quadratic_objective_*!, p_terms)
//   kind 3  parameter×variable term (p, v = i) of the objective (pv_terms)
// Reverse (parameters.jl:341-534):  dp[p] += c · s(t) with s the reverse getter
//   value the reference reads: kind 0 the constant of ReverseConstraintFunction
//   (λ_i·dλ_i), kind 1 its constant (dν_i), kind 2 the constant of
//   ReverseObjectiveFunction (0.0, QuadraticProgram.jl:448-458), kind 3 the
//   coefficient of v in it (dz_v).  The objective's parameter×parameter terms
//   multiply that same constant (0.0) and contribute nothing.
// Forward (parameters.jl:91-300):  the constraint / objective tangents
//   cte(row) += dp[p] · c, pv: coefficient of v += dp[p] · c, returned in the
//   engine's forward inputs: dh_i = −cte (LessThan), db_i = −cte (EqualTo) —
//   the `_fill` negation of MOI constants (diff_opt.jl:616-622) — and dq_v.
//   The objective's constant tangent does not enter the KKT system.
// Each sum runs over its terms in the order the caller lists them (the
// reference's accumulation order when the caller preserves it).
// The `_k` calls ("QP parameter calls on k seeds" below) add
//   kind 4  parameter×variable term (p, v) of LessThan row i  (ParametricQuadraticFunction
//   kind 5  parameter×variable term (p, v) of EqualTo row i    constraints, :147-203, :390-441)
// whose forward tangent is dG[i, v] / dA[i, v] += dp[p] · c and whose reverse
// getter is the coefficient of v in ReverseConstraintFunction(ci).
#include "dopt_internal.h"

#include <algorithm>
#include <numeric>

namespace dopt {

namespace {

constexpr int PTPB = 256;

// one thread per (problem, output row); CSR by output row
__global__ __launch_bounds__(PTPB) void poi_reverse_kernel(const double* __restrict__ rev,
                                                           const double* __restrict__ lam, int n, int m, int p,
                                                           int nparam, const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ kind,
                                                           const int32_t* __restrict__ index,
                                                           const double* __restrict__ coef,
                                                           double* __restrict__ out) {
  const int b = blockIdx.y, r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= nparam) return;
  const double* rv = rev + (size_t)b * (n + m + p);
  double acc = 0.0;
  for (int64_t t = ptr[r]; t < ptr[r + 1]; ++t) {
    const int i = index[t];
    double s;
    switch (kind[t]) {
      case 0: s = lam[(size_t)b * m + i] * rv[n + i]; break;   // λ_i·dλ_i
      case 1: s = rv[n + m + i]; break;                         // dν_i
      case 3: s = rv[i]; break;                                 // dz_v
      default: s = 0.0; break;                                  // objective constant
    }
    acc += coef[t] * s;
  }
  out[(size_t)b * nparam + r] = acc;
}

__global__ __launch_bounds__(PTPB) void poi_forward_kernel(const double* __restrict__ dp, int nparam, int n,
                                                           int m, int p, const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ param,
                                                           const double* __restrict__ coef,
                                                           double* __restrict__ dq, double* __restrict__ dh,
                                                           double* __restrict__ db) {
  const int b = blockIdx.y, r = blockIdx.x * PTPB + threadIdx.x;   // r: m LE rows | p EQ rows | n variables
  if (r >= m + p + n) return;
  double acc = 0.0;
  for (int64_t t = ptr[r]; t < ptr[r + 1]; ++t) acc += dp[(size_t)b * nparam + param[t]] * coef[t];
  if (r < m) dh[(size_t)b * m + r] = -acc;
  else if (r < m + p) db[(size_t)b * p + (r - m)] = -acc;
  else dq[(size_t)b * n + (r - m - p)] = acc;
}

// ---------------------------------------------------------------------------
// QP parameter calls on k seeds (dopt_qp_params_forward_k / _reverse_k).  A
// column is one (seed, problem) pair, seed-major: column c = seed·B + b works
// on problem b = c mod B; work vectors at + c·nmax, outputs at + c·(n+m+p).
// ---------------------------------------------------------------------------
// The tangent of term (param, coef) in column c: dp·c, or for the unit seeds
// (dp == null) the same product on the unit vector of parameter `unit`.
__device__ __forceinline__ double poi_dt(const double* __restrict__ dp, size_t c, int nparam, int unit, int param,
                                         double coef) {
  return (dp ? dp[c * nparam + param] : (param == unit ? 1.0 : 0.0)) * coef;
}

// λ·a − λ·b with both products rounded, as Julia's λ.*(dG z) − λ.*dh rounds
// them (no contraction into an FMA): equal a and b cancel exactly, so a
// direction the problem does not move along gives an exactly zero entry.
__device__ __forceinline__ double lam_diff(double l, double a, double b) {
#pragma clang fp contract(off)
  return l * a - l * b;
}

// Forward right-hand sides of a chunk of seeds, straight from the term table
// (parameters.jl:91-300 into QuadraticProgram.jl:429-433): what
// qp_fwd_rhs_kernel (qp.hip) writes from the dense tangents the terms define —
// dq_v = Σ d (kind 3), dh_i = −Σ d (kind 0), db_e = −Σ d (kind 1),
// dG[i,v] = Σ d (kind 4), dA[e,v] = Σ d (kind 5), d = dp·c — with its
// expression shapes (the transposed products added to dq one after the other,
// λ·(dG z) − λ·dh, dA z − db), and both of its copies: the full-length one
// (`full`; the output kernel recovers an eliminated row's x_λ as r_i/s_i from
// it) and the reduced one (`rhs`, through rpos and meta.nk).  One thread per
// (row, column); rows [0, nmax): every entry of both copies is written (zeros
// past n+m+p and past the reduced size), the buffers being reused between
// calls.  Two CSRs over the terms, each stable in the caller's order: `r*` by
// constraint row (m LessThan rows, then p EqualTo rows; kinds 0, 1, 4, 5),
// `v*` by variable (kinds 3, 4, 5; `vindex` the term's row).
__global__ __launch_bounds__(PTPB) void qp_poi_fwd_rhs_kernel(
    const double* __restrict__ dp, int p0, int nparam, int n, int m, int p, int nmax, int B, int64_t cols,
    const int64_t* __restrict__ rptr, const int32_t* __restrict__ rkind, const int32_t* __restrict__ rparam,
    const int32_t* __restrict__ rvar, const double* __restrict__ rcoef, const int64_t* __restrict__ vptr,
    const int32_t* __restrict__ vkind, const int32_t* __restrict__ vparam, const int32_t* __restrict__ vindex,
    const double* __restrict__ vcoef, const double* __restrict__ z, const double* __restrict__ lam,
    const double* __restrict__ nu, const int32_t* __restrict__ rpos, const QPMeta* __restrict__ meta,
    double* __restrict__ full, double* __restrict__ rhs) {
  const int r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= nmax) return;
  const int L = n + m + p;
  int64_t t0 = 0, t1 = 0;
  if (r < n) {
    t0 = vptr[r];
    t1 = vptr[r + 1];
  } else if (r < L) {
    t0 = rptr[r - n];
    t1 = rptr[r - n + 1];
  }
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    const int b = (int)(c % B), unit = p0 + (int)(c / B);
    const double* zb = z + (size_t)b * n;
    const double* lb = lam + (size_t)b * m;
    const double* nb = nu + (size_t)b * p;
    double val = 0.0;
    int dst = -1;   // the entry's place in the reduced system (−1: an eliminated row, or padding)
    if (r < n) {
      // r1 = dq + dGᵀλ + dAᵀν
      double aq = 0.0, ag = 0.0, aa = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        const double d = poi_dt(dp, (size_t)c, nparam, unit, vparam[t], vcoef[t]);
        const int k = vkind[t];
        if (k == 3) aq += d;
        else if (k == 4) ag = fma(d, lb[vindex[t]], ag);
        else aa = fma(d, nb[vindex[t]], aa);
      }
      val = aq;
      val += ag;
      val += aa;
      dst = r;
    } else if (r < n + m) {
      // r2 = λ.*(dG z) − λ.*dh
      const int l = r - n;
      double gz = 0.0, cte = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        const double d = poi_dt(dp, (size_t)c, nparam, unit, rparam[t], rcoef[t]);
        if (rkind[t] == 4) gz = fma(d, zb[rvar[t]], gz);
        else cte += d;
      }
      const double hh = -cte;
      val = lam_diff(lb[l], gz, hh);
      const int kk = rpos[(size_t)b * m + l];
      if (kk >= 0) dst = n + kk;
    } else if (r < L) {
      // r3 = dA z − db
      double az = 0.0, cte = 0.0;
      for (int64_t t = t0; t < t1; ++t) {
        const double d = poi_dt(dp, (size_t)c, nparam, unit, rparam[t], rcoef[t]);
        if (rkind[t] == 5) az = fma(d, zb[rvar[t]], az);
        else cte += d;
      }
      val = az - (-cte);
      dst = n + meta[b].nk + (r - n - m);
    }
    full[(size_t)c * nmax + r] = val;
    if (dst >= 0) rhs[(size_t)c * nmax + dst] = val;   // dst < nsys: no two threads share an entry
    if (r >= meta[b].nsys) rhs[(size_t)c * nmax + r] = 0.0;
  }
}

// Reverse right-hand sides of a chunk of seeds: [dl_dz; 0] of the column
// (what qp_rev_rhs_kernel, qp.hip, writes), or for the unit seeds (dl_dz ==
// null) e_{v0 + seed}.  Rows [0, nmax): no stale entry.
__global__ __launch_bounds__(PTPB) void qp_poi_rev_rhs_kernel(const double* __restrict__ dl_dz, int v0, int n,
                                                              int nmax, int B, int64_t cols,
                                                              double* __restrict__ rhs) {
  const int i = blockIdx.x * PTPB + threadIdx.x;
  if (i >= nmax) return;
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    double v = 0.0;
    if (i < n) v = dl_dz ? dl_dz[(size_t)c * n + i] : (i == v0 + (int)(c / B) ? 1.0 : 0.0);
    rhs[(size_t)c * nmax + i] = v;
  }
}

// Reverse right-hand sides of a chunk of seeds with a loss gradient on the
// duals too: [g_z; g_λ; g_ν] of the column (a null block is zero).  The
// full-length copy (`full`, rows [0, nmax): zeros past n+m+p) is what the
// output kernel reads an eliminated row's g_λ from; the reduced copy (`rhs`)
// goes through rpos and meta.nk as qp_fwd_rhs_kernel (qp.hip) scatters its
// rows, and only its entries < nsys are written, as qp_rev_rhs_kernel does.
__global__ __launch_bounds__(PTPB) void qp_rev_rhs_duals_kernel(
    const double* __restrict__ g_z, const double* __restrict__ g_lam, const double* __restrict__ g_nu, int n, int m,
    int p, int nmax, int B, int64_t cols, const int32_t* __restrict__ rpos, const QPMeta* __restrict__ meta,
    double* __restrict__ full, double* __restrict__ rhs) {
  const int r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= nmax) return;
  const int L = n + m + p;
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    const int b = (int)(c % B);
    double v = 0.0;
    int dst = -1;   // the entry's place in the reduced system (−1: an eliminated row, or padding)
    if (r < n) {
      if (g_z) v = g_z[(size_t)c * n + r];
      dst = r;
    } else if (r < n + m) {
      const int l = r - n;
      if (g_lam) v = g_lam[(size_t)c * m + l];
      const int kk = rpos[(size_t)b * m + l];
      if (kk >= 0) dst = n + kk;
    } else if (r < L) {
      const int e = r - n - m;
      if (g_nu) v = g_nu[(size_t)c * p + e];
      dst = n + meta[b].nk + e;
    }
    full[(size_t)c * nmax + r] = v;
    if (dst >= 0) rhs[(size_t)c * nmax + dst] = v;   // dst < nsys: no two threads share an entry
  }
}

// Reverse accumulation over the columns (parameters.jl:341-534): one thread
// per (column, parameter), out[c·nparam + r] = Σ_t c_t·s_t over the
// parameter's terms in the caller's order, from the column's full reverse
// output rev = [dz | dλ | dν] (qp_output_k_kernel's, the eliminated rows' dλ
// included).  Kinds 0-3 as poi_reverse_kernel.  Kinds 4 and 5 read the
// coefficient of v in ReverseConstraintFunction(ci) (:390-441): the entry
// expressions restate qp_reverse_grads_kernel's dG / dA (qp.hip) — change
// them together:
//   kind 4  s = λ_i·dλ_i·z_v + λ_i·dz_v
//   kind 5  s = dν_i·z_v + ν_i·dz_v
__global__ __launch_bounds__(PTPB) void qp_poi_reverse_k_kernel(
    const double* __restrict__ rev, const double* __restrict__ z, const double* __restrict__ lam,
    const double* __restrict__ nu, int n, int m, int p, int B, int64_t cols, int nparam,
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ kind, const int32_t* __restrict__ index,
    const int32_t* __restrict__ var, const double* __restrict__ coef, double* __restrict__ out) {
  const int r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= nparam) return;
  const int L = n + m + p;
  const int64_t t0 = ptr[r], t1 = ptr[r + 1];
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    const int b = (int)(c % B);
    const double* rb = rev + (size_t)c * L;
    const double* zb = z + (size_t)b * n;
    const double* lb = lam + (size_t)b * m;
    const double* nb = nu + (size_t)b * p;
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
      const int i = index[t];
      double s;
      switch (kind[t]) {
        case 0: s = lb[i] * rb[n + i]; break;   // λ_i·dλ_i
        case 1: s = rb[n + m + i]; break;       // dν_i
        case 3: s = rb[i]; break;               // dz_v
        case 4: {
          const int j = var[t];
          const double li = lb[i];
          s = li * rb[n + i] * zb[j] + li * rb[j];
          break;
        }
        case 5: {
          const int j = var[t];
          s = rb[n + m + i] * zb[j] + nb[i] * rb[j];
          break;
        }
        default: s = 0.0; break;                // objective constant
      }
      acc += coef[t] * s;
    }
    out[(size_t)c * nparam + r] = acc;
  }
}

// ---------------------------------------------------------------------------
// Conic parameter accumulation (parameters.jl:341-534 consuming
// ConicProgram.jl:396-443).  Kinds keep the QP numbers where they mean the
// same: 0 parameter term of constraint row i ∈ [0, m) in ProductOfSets order
// (ParametricVectorAffineFunction), 2 parameter term of the objective, 3
// parameter×variable term of the objective; 1 does not exist here.
// A column is one (seed, problem) pair, seed-major as every _k array: column
// c = seed·B + b reads problem b = c mod B's x and vp.  A single call has one
// seed (cols = B); the Jacobian's chunks have k.
// ---------------------------------------------------------------------------
// Forward (parameters.jl:120-145, :226-275, then ConicProgram.jl:270-287):
// one thread per (column, output row), rows = m constraint rows then n
// variables; db_i = +Σ c·dp (the conic `_fill` runs with S -> false: no
// negation, unlike the QP's dh / db), dc_v = Σ c·dp.  dp == null: the
// column's tangent is the unit vector of parameter p0 + seed (the Jacobian's
// seeds; the same products and sums as the call on that unit dp).
__global__ __launch_bounds__(PTPB) void conic_poi_forward_kernel(const double* __restrict__ dp, int p0, int nparam,
                                                                 int n, int m, int B, int64_t cols,
                                                                 const int64_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ param,
                                                                 const double* __restrict__ coef,
                                                                 double* __restrict__ db, double* __restrict__ dc) {
  const int r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= m + n) return;
  const int64_t t0 = ptr[r], t1 = ptr[r + 1];
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    const int unit = p0 + (int)(c / B);
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
      const double d = dp ? dp[(size_t)c * nparam + param[t]] : (param[t] == unit ? 1.0 : 0.0);
      acc += d * coef[t];
    }
    if (r < m) db[(size_t)c * m + r] = acc;
    else dc[(size_t)c * n + (r - m)] = acc;
  }
}

// Reverse (parameters.jl:365-388, :463-509): one thread per (column,
// parameter), out[c·nparam + p] = Σ_t c_t·s_t over the parameter's terms in
// the caller's order.  The two entry expressions restate conic_rev_out_kernel's
// out_db / out_dc (conic.hip) — change them together:
//   kind 0  s = g[n+i] − g[n+m]·vp[i]   (_get_db, ConicProgram.jl:414-428)
//   kind 3  s = g[v]   − g[n+m]·x[v]    (ReverseObjectiveFunction's coefficient of v, :396-401)
//   kind 2  s = 0                       (its constant is 0.0, :400)
__global__ __launch_bounds__(PTPB) void conic_poi_reverse_kernel(const double* __restrict__ g,
                                                                 const double* __restrict__ x,
                                                                 const double* __restrict__ vp, int n, int m, int B,
                                                                 int64_t cols, int nparam,
                                                                 const int64_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ kind,
                                                                 const int32_t* __restrict__ index,
                                                                 const double* __restrict__ coef,
                                                                 double* __restrict__ out) {
  const int r = blockIdx.x * PTPB + threadIdx.x;
  if (r >= nparam) return;
  const int N = n + m + 1;
  const int64_t t0 = ptr[r], t1 = ptr[r + 1];
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) {
    const int b = (int)(c % B);
    const double* gb = g + (size_t)c * N;
    const double* xb = x + (size_t)b * n;
    const double* vpb = vp + (size_t)b * m;
    const double ge = gb[N - 1];
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
      const int i = index[t];
      double s;
      switch (kind[t]) {
        case 0: s = gb[n + i] - ge * vpb[i]; break;
        case 3: s = gb[i] - ge * xb[i]; break;
        default: s = 0.0; break;
      }
      acc += coef[t] * s;
    }
    out[(size_t)c * nparam + r] = acc;
  }
}

// the Jacobian's reverse seeds: column c = seed·B + b gets the unit vector of variable v0 + seed
__global__ __launch_bounds__(PTPB) void conic_unit_seed_kernel(int v0, int n, int B, int64_t cols,
                                                               double* __restrict__ dx) {
  const int v = blockIdx.x * PTPB + threadIdx.x;
  if (v >= n) return;
  for (int64_t c = blockIdx.y; c < cols; c += gridDim.y) dx[(size_t)c * n + v] = v == v0 + (int)(c / B) ? 1.0 : 0.0;
}

struct Csr {
  std::vector<int64_t> ptr;
  std::vector<int32_t> kind, index, param;
  std::vector<int32_t> var;   // kinds 4 and 5: the term's variable (the _k calls; empty otherwise)
  std::vector<double> coef;
};

// t_var: the variables of the constraints' parameter×variable terms (kinds 4: LessThan row, 5: EqualTo row), which
// only the _k calls take (pv); without pv kinds above 3 are out of range
void validate(const Handle& h, int nparam, int64_t nterms, const int32_t* t_param, const int32_t* t_kind,
              const int32_t* t_index, const double* t_coef, const int32_t* t_var = nullptr, bool pv = false) {
  if (nparam < 0 || nterms < 0) throw Error(-1, "parameter accumulation: negative size");
  if (nterms > 0 && (!t_param || !t_kind || !t_index || !t_coef))
    throw Error(-1, "parameter accumulation: term arrays are required");
  for (int64_t t = 0; t < nterms; ++t) {
    const int k = t_kind[t], i = t_index[t];
    const bool var = pv && (k == 4 || k == 5);
    if (var && !t_var)
      throw Error(-1, "parameter accumulation: term " + std::to_string(t) + " of kind " + std::to_string(k) +
                          " needs t_var");
    const int lim = k == 0 || k == 4 ? h.m : k == 1 || k == 5 ? h.p : k == 3 ? h.n : 1;
    if (t_param[t] < 0 || t_param[t] >= nparam || k < 0 || k > (pv ? 5 : 3) || (k != 2 && (i < 0 || i >= lim)) ||
        (var && (t_var[t] < 0 || t_var[t] >= h.n)))
      throw Error(-1, "parameter accumulation: term " + std::to_string(t) + " out of range");
  }
}

void validate_conic(const Handle& h, int nparam, int64_t nterms, const int32_t* t_param, const int32_t* t_kind,
                    const int32_t* t_index, const double* t_coef) {
  if (nparam < 0 || nterms < 0) throw Error(-1, "parameter accumulation: negative size");
  if (nterms > 0 && (!t_param || !t_kind || !t_index || !t_coef))
    throw Error(-1, "parameter accumulation: term arrays are required");
  for (int64_t t = 0; t < nterms; ++t) {
    const int k = t_kind[t], i = t_index[t];
    const int lim = k == 0 ? h.m : h.n;
    if (t_param[t] < 0 || t_param[t] >= nparam || (k != 0 && k != 2 && k != 3) || (k != 2 && (i < 0 || i >= lim)))
      throw Error(-1, "parameter accumulation: term " + std::to_string(t) + " out of range");
  }
}

// stable CSR by `key` (terms keep their relative order within a row)
Csr csr_by(int rows, int64_t nterms, const std::vector<int32_t>& key, const int32_t* t_param,
           const int32_t* t_kind, const int32_t* t_index, const double* t_coef, const int32_t* t_var = nullptr) {
  Csr c;
  c.ptr.assign(rows + 1, 0);
  for (int64_t t = 0; t < nterms; ++t) ++c.ptr[key[t] + 1];
  std::partial_sum(c.ptr.begin(), c.ptr.end(), c.ptr.begin());
  std::vector<int64_t> pos(c.ptr.begin(), c.ptr.end() - 1);
  c.kind.resize(nterms);
  c.index.resize(nterms);
  c.param.resize(nterms);
  c.coef.resize(nterms);
  if (t_var) c.var.resize(nterms);
  for (int64_t t = 0; t < nterms; ++t) {
    const int64_t d = pos[key[t]]++;
    if (t_var) c.var[d] = t_var[t];
    c.kind[d] = t_kind[t];
    c.index[d] = t_index[t];
    c.param[d] = t_param[t];
    c.coef[d] = t_coef[t];
  }
  return c;
}

// the CSR arrays in the handle's term-table buffer (h.pterms grows like every
// staging buffer).  The copies read `c`: every caller waits for the stream
// before `c` goes out of scope.
struct DevCsr {
  int64_t* ptr = nullptr;
  int32_t *kind = nullptr, *index = nullptr, *param = nullptr, *var = nullptr;
  double* coef = nullptr;
  DevCsr() = default;
  DevCsr(Handle& h, const Csr& c) {
    h.pterms.ensure(bytes(c));
    place(h, c, h.pterms.as<char>());
  }
  static size_t bytes(const Csr& c) {
    const size_t nt = c.coef.size(), np = c.ptr.size();
    return (np * 8 + nt * 8 + 4 * nt * 4 + 64 + 63) / 64 * 64;
  }
  // the arrays at `p` (inside h.pterms, bytes(c) long), copies queued on the handle's stream
  void place(Handle& h, const Csr& c, char* p) {
    const hipStream_t st = h.stream;
    const size_t nt = c.coef.size(), np = c.ptr.size();
    ptr = reinterpret_cast<int64_t*>(p);
    coef = reinterpret_cast<double*>(p + np * 8);
    kind = reinterpret_cast<int32_t*>(p + np * 8 + nt * 8);
    index = kind + nt;
    param = index + nt;
    var = param + nt;
    DOPT_CHECK_HIP(hipMemcpyAsync(ptr, c.ptr.data(), np * 8, hipMemcpyHostToDevice, st));
    if (nt) {
      DOPT_CHECK_HIP(hipMemcpyAsync(coef, c.coef.data(), nt * 8, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(kind, c.kind.data(), nt * 4, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(index, c.index.data(), nt * 4, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(param, c.param.data(), nt * 4, hipMemcpyHostToDevice, st));
      if (!c.var.empty()) DOPT_CHECK_HIP(hipMemcpyAsync(var, c.var.data(), nt * 4, hipMemcpyHostToDevice, st));
    }
  }
};

}  // namespace

void qp_params_reverse(Handle& h, const double* rev, int nparam, int64_t nterms, const int32_t* t_param,
                       const int32_t* t_kind, const int32_t* t_index, const double* t_coef, double* out) {
  if (!h.set) throw Error(-1, "dopt_qp_params_reverse: dopt_qp_set has not been called");
  validate(h, nparam, nterms, t_param, t_kind, t_index, t_coef);
  if (nparam == 0) return;
  std::vector<int32_t> key(t_param, t_param + nterms);
  const Csr c = csr_by(nparam, nterms, key, t_param, t_kind, t_index, t_coef);
  DevCsr d(h, c);
  static const double dummy = 0.0;
  hipLaunchKernelGGL(poi_reverse_kernel, dim3((nparam + PTPB - 1) / PTPB, (unsigned)h.batch), dim3(PTPB), 0,
                     h.stream, rev, h.m ? h.lam : &dummy, h.n, h.m, h.p, nparam, d.ptr, d.kind, d.index, d.coef,
                     out);
  DOPT_CHECK_HIP(hipGetLastError());
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));   // the copies out of `c` are done
}

void qp_params_forward(Handle& h, const double* dp, int nparam, int64_t nterms, const int32_t* t_param,
                       const int32_t* t_kind, const int32_t* t_index, const double* t_coef, double* dq,
                       double* dh, double* db) {
  if (!h.set) throw Error(-1, "dopt_qp_params_forward: dopt_qp_set has not been called");
  validate(h, nparam, nterms, t_param, t_kind, t_index, t_coef);
  const int rows = h.m + h.p + h.n;
  std::vector<int32_t> key(nterms);
  std::vector<int32_t> kind(nterms);
  for (int64_t t = 0; t < nterms; ++t) {   // objective constants (kind 2) are dropped
    const int k = t_kind[t], i = t_index[t];
    key[t] = k == 0 ? i : k == 1 ? h.m + i : k == 3 ? h.m + h.p + i : -1;
  }
  std::vector<int64_t> keep;
  for (int64_t t = 0; t < nterms; ++t)
    if (key[t] >= 0) keep.push_back(t);
  std::vector<int32_t> k2(keep.size()), p2(keep.size()), i2(keep.size()), kk(keep.size());
  std::vector<double> c2(keep.size());
  for (size_t u = 0; u < keep.size(); ++u) {
    kk[u] = key[keep[u]];
    p2[u] = t_param[keep[u]];
    k2[u] = t_kind[keep[u]];
    i2[u] = t_index[keep[u]];
    c2[u] = t_coef[keep[u]];
  }
  const Csr c = csr_by(rows, (int64_t)keep.size(), kk, p2.data(), k2.data(), i2.data(), c2.data());
  DevCsr d(h, c);
  static double dummy = 0.0;
  hipLaunchKernelGGL(poi_forward_kernel, dim3((rows + PTPB - 1) / PTPB, (unsigned)h.batch), dim3(PTPB), 0,
                     h.stream, dp, std::max(nparam, 1), h.n, h.m, h.p, d.ptr, d.param, d.coef, dq,
                     h.m ? dh : &dummy, h.p ? db : &dummy);
  DOPT_CHECK_HIP(hipGetLastError());
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));
}

// ---------------------------------------------------------------------------
// conic parameter accumulation: host side
// ---------------------------------------------------------------------------
namespace {

// the terms that enter the forward tangents (kinds 0 and 3; kind 2 is dropped), by output row: m constraint rows,
// then n variables
Csr conic_forward_csr(const Handle& h, int64_t nterms, const int32_t* t_param, const int32_t* t_kind,
                      const int32_t* t_index, const double* t_coef) {
  std::vector<int32_t> key, p2, k2, i2;
  std::vector<double> c2;
  for (int64_t t = 0; t < nterms; ++t) {
    if (t_kind[t] == 2) continue;
    key.push_back(t_kind[t] == 0 ? t_index[t] : h.m + t_index[t]);
    p2.push_back(t_param[t]);
    k2.push_back(t_kind[t]);
    i2.push_back(t_index[t]);
    c2.push_back(t_coef[t]);
  }
  return csr_by(h.m + h.n, (int64_t)key.size(), key, p2.data(), k2.data(), i2.data(), c2.data());
}

dim3 poi_grid(int rows, int64_t cols) {
  return dim3((unsigned)((rows + PTPB - 1) / PTPB), (unsigned)std::min<int64_t>(std::max<int64_t>(cols, 1), 65535));
}

void launch_conic_forward(Handle& h, const DevCsr& d, const double* dp, int p0, int nparam, int64_t cols, double* db,
                          double* dc) {
  const int rows = h.m + h.n;
  if (rows == 0 || cols == 0) return;
  hipLaunchKernelGGL(conic_poi_forward_kernel, poi_grid(rows, cols), dim3(PTPB), 0, h.stream, dp, p0,
                     std::max(nparam, 1), h.n, h.m, (int)h.batch, cols, d.ptr, d.param, d.coef, db, dc);
  DOPT_CHECK_HIP(hipGetLastError());
}

void launch_conic_reverse(Handle& h, const DevCsr& d, const double* g, int nparam, int64_t cols, double* out) {
  if (nparam == 0 || cols == 0) return;
  const double* vp = h.vp.as<double>() + (size_t)h.batch * h.m;
  hipLaunchKernelGGL(conic_poi_reverse_kernel, poi_grid(nparam, cols), dim3(PTPB), 0, h.stream, g, h.cx, vp, h.n,
                     h.m, (int)h.batch, cols, nparam, d.ptr, d.kind, d.index, d.coef, out);
  DOPT_CHECK_HIP(hipGetLastError());
}

// Seeds per chunk of the Jacobian.  One seed of one call costs, per problem,
// the LSQR workspace conic_run sizes (conic_seed_doubles: 6N + 3m + n), its
// materialised tangents or seed (m + n, or n) and its LSQR solution (N):
// at most 7N + 4m + 2n doubles.  The chunk is the largest multiple of the
// seed group (so every group but the call's last is full) that keeps
// chunk · B · that within JAC_WS_BYTES, and at least one group.
// DOPT_CONIC_JAC_CHUNK=<k ≥ 1> overrides it (the tests' chunk edges).
constexpr size_t JAC_WS_BYTES = (size_t)1 << 30;
int jacobian_chunk(const Handle& h, int seeds) {
  if (const char* e = getenv("DOPT_CONIC_JAC_CHUNK")) {
    const int k = atoi(e);
    if (k >= 1) return std::min(k, seeds);
  }
  const size_t per_seed = std::max<size_t>(h.batch, 1) * (conic_seed_doubles(h) + 2 * ((size_t)h.n + h.m) + 1) *
                          sizeof(double);
  const int G = conic_seed_group();
  const size_t fit = JAC_WS_BYTES / per_seed / G * G;
  return (int)std::min<size_t>(std::max<size_t>(fit, G), (size_t)seeds);
}

}  // namespace

// ---------------------------------------------------------------------------
// QP parameter calls on k seeds: host side
// ---------------------------------------------------------------------------
namespace {

// Seeds per chunk.  One seed costs, per problem, its reduced right-hand side,
// solution and full forward copy (krhs + kx + kfull: 3·nmax doubles) and, in
// reverse without out_rev, its outputs in the handle's scratch (n+m+p).  The
// chunk is the largest multiple of 16 (the multi-RHS kernel's seed group and
// the output kernel's) that keeps chunk · B · that within JAC_WS_BYTES, and at
// least 16.  DOPT_QP_JAC_CHUNK=<k ≥ 1> overrides it (the tests' chunk edges).
int qp_jacobian_chunk(const Handle& h, int seeds) {
  if (const char* e = getenv("DOPT_QP_JAC_CHUNK")) {
    const int k = atoi(e);
    if (k >= 1) return std::min(k, seeds);
  }
  constexpr size_t G = 16;
  const size_t per_seed = std::max<size_t>(h.batch, 1) * (3 * (size_t)h.nmax + h.n + h.m + h.p) * sizeof(double);
  const size_t fit = JAC_WS_BYTES / per_seed / G * G;
  return (int)std::min<size_t>(std::max<size_t>(fit, G), (size_t)seeds);
}

void qp_k_checks(Handle& h, const char* fn) {
  if (!h.set) throw Error(-1, std::string(fn) + ": dopt_qp_set has not been called");
  if (h.sparse) throw Error(-1, "multi-RHS calls need factors: not on the sparse (LSQR) route");
}

const int32_t* qp_rpos(Handle& h) { return h.kidx.as<int32_t>() + (size_t)h.batch * h.m; }

}  // namespace

void qp_params_forward_k(Handle& h, int k, const double* dp, int nparam, int64_t nterms, const int32_t* t_param,
                         const int32_t* t_kind, const int32_t* t_index, const int32_t* t_var, const double* t_coef,
                         double* out) {
  qp_k_checks(h, "dopt_qp_params_forward_k");
  if (k < 0) throw Error(-1, "dopt_qp_params_forward_k: k must not be negative");
  validate(h, nparam, nterms, t_param, t_kind, t_index, t_coef, t_var, true);
  if (nparam == 0 || k == 0 || h.batch == 0) return;
  if (!out) throw Error(-1, "dopt_qp_params_forward_k: out is required");
  if (!h.factored) qp_factor(h);
  const int n = h.n, m = h.m, p = h.p, nmax = h.nmax;
  const size_t B = h.batch, L = (size_t)n + m + p, blk = B * nmax;
  // by constraint row (kinds 0, 1, 4, 5) and by variable (kinds 3, 4, 5); kind 2 is dropped
  std::vector<int32_t> rkey, rpar, rkind, ridx, rvar, vkey, vpar, vkind, vidx, vvar;
  std::vector<double> rco, vco;
  for (int64_t t = 0; t < nterms; ++t) {
    const int kd = t_kind[t], i = t_index[t], v = kd == 4 || kd == 5 ? t_var[t] : 0;
    if (kd == 0 || kd == 1 || kd == 4 || kd == 5) {
      rkey.push_back(kd == 0 || kd == 4 ? i : m + i);
      rpar.push_back(t_param[t]);
      rkind.push_back(kd);
      ridx.push_back(i);
      rvar.push_back(v);
      rco.push_back(t_coef[t]);
    }
    if (kd == 3 || kd == 4 || kd == 5) {
      vkey.push_back(kd == 3 ? i : v);
      vpar.push_back(t_param[t]);
      vkind.push_back(kd);
      vidx.push_back(i);
      vvar.push_back(v);
      vco.push_back(t_coef[t]);
    }
  }
  const Csr cr = csr_by(m + p, (int64_t)rkey.size(), rkey, rpar.data(), rkind.data(), ridx.data(), rco.data(),
                        rvar.data());
  const Csr cv = csr_by(n, (int64_t)vkey.size(), vkey, vpar.data(), vkind.data(), vidx.data(), vco.data(),
                        vvar.data());
  h.pterms.ensure(DevCsr::bytes(cr) + DevCsr::bytes(cv));
  DevCsr dr, dv;
  dr.place(h, cr, h.pterms.as<char>());
  dv.place(h, cv, h.pterms.as<char>() + DevCsr::bytes(cr));
  const int chunk = qp_jacobian_chunk(h, k);
  h.krhs.ensure((size_t)chunk * blk * sizeof(double));
  h.kx.ensure((size_t)chunk * blk * sizeof(double));
  h.kfull.ensure((size_t)chunk * blk * sizeof(double));
  double* rk = h.krhs.as<double>();
  double* xk = h.kx.as<double>();
  double* fk = h.kfull.as<double>();
  static const double dummy = 0.0;
  for (int s0 = 0; s0 < k; s0 += chunk) {
    const int kc = std::min(chunk, k - s0);
    const int64_t cols = (int64_t)kc * (int64_t)B;
    {
      PhaseTimer pt(h, DOPT_PHASE_QP_RHS);
      hipLaunchKernelGGL(qp_poi_fwd_rhs_kernel, poi_grid(nmax, cols), dim3(PTPB), 0, h.stream,
                         dp ? dp + (size_t)s0 * B * nparam : nullptr, s0, nparam, n, m, p, nmax, (int)B, cols, dr.ptr,
                         dr.kind, dr.param, dr.var, dr.coef, dv.ptr, dv.kind, dv.param, dv.index, dv.coef, h.z,
                         m ? h.lam : &dummy, p ? h.nu : &dummy, qp_rpos(h), h.meta.as<QPMeta>(), fk, rk);
      DOPT_CHECK_HIP(hipGetLastError());
    }
    solve_k(h, 1, kc, rk, xk, fk, out + (size_t)s0 * B * L);
  }
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));   // the copies out of `cr` / `cv` are done
}

namespace {

// The seeds of a reverse call on k columns.  duals: the loss gradient has λ /
// ν blocks (a null pointer is a zero block) and the right-hand sides are
// qp_rev_rhs_duals_kernel's; otherwise [dl_dz; 0] or the unit seeds
// (qp_poi_rev_rhs_kernel).
struct RevSeeds {
  const double* z;
  const double* lam;
  const double* nu;
  bool duals;
};

// The chunk loop of the reverse `_k` calls on kept factors: per chunk of
// qp_jacobian_chunk seeds the right-hand sides, solve_k into the chunk's place
// in out_rev (null: the handle's scratch, overwritten by the next chunk), then
// after(s0, cols, rev) on the chunk's outputs.
template <class After>
void qp_reverse_chunks(Handle& h, int k, const RevSeeds& g, double* out_rev, After&& after) {
  const int n = h.n, m = h.m, p = h.p, nmax = h.nmax;
  const size_t B = h.batch, L = (size_t)n + m + p, blk = B * nmax;
  const int chunk = qp_jacobian_chunk(h, k);
  h.krhs.ensure((size_t)chunk * blk * sizeof(double));
  h.kx.ensure((size_t)chunk * blk * sizeof(double));
  if (g.duals) h.kfull.ensure((size_t)chunk * blk * sizeof(double));
  if (!out_rev) h.qjac.ensure((size_t)chunk * B * L * sizeof(double));
  double* rk = h.krhs.as<double>();
  double* xk = h.kx.as<double>();
  double* fk = g.duals ? h.kfull.as<double>() : nullptr;
  for (int s0 = 0; s0 < k; s0 += chunk) {
    const int kc = std::min(chunk, k - s0);
    const int64_t cols = (int64_t)kc * (int64_t)B;
    auto at = [&](const double* a, int len) { return a ? a + (size_t)s0 * B * len : nullptr; };
    {
      PhaseTimer pt(h, DOPT_PHASE_QP_RHS);
      if (g.duals)
        hipLaunchKernelGGL(qp_rev_rhs_duals_kernel, poi_grid(nmax, cols), dim3(PTPB), 0, h.stream, at(g.z, n),
                           m ? at(g.lam, m) : nullptr, p ? at(g.nu, p) : nullptr, n, m, p, nmax, (int)B, cols,
                           qp_rpos(h), h.meta.as<QPMeta>(), fk, rk);
      else
        hipLaunchKernelGGL(qp_poi_rev_rhs_kernel, poi_grid(nmax, cols), dim3(PTPB), 0, h.stream, at(g.z, n), s0, n,
                           nmax, (int)B, cols, rk);
      DOPT_CHECK_HIP(hipGetLastError());
    }
    double* rev = out_rev ? out_rev + (size_t)s0 * B * L : h.qjac.as<double>();
    solve_k(h, 0, kc, rk, xk, fk, rev, g.duals);
    after(s0, cols, rev);
  }
}

// The parameter gradients of the reverse `_k` calls: the term table by
// parameter, then qp_poi_reverse_k_kernel over every chunk's reverse outputs.
void qp_params_reverse_chunks(Handle& h, int k, const RevSeeds& g, int nparam, int64_t nterms, const int32_t* t_param,
                              const int32_t* t_kind, const int32_t* t_index, const int32_t* t_var,
                              const double* t_coef, double* out_rev, double* out_dp) {
  const int n = h.n, m = h.m, p = h.p;
  const size_t B = h.batch;
  std::vector<int32_t> var(nterms, 0);
  for (int64_t t = 0; t < nterms; ++t)
    if (t_kind[t] == 4 || t_kind[t] == 5) var[t] = t_var[t];
  const Csr c = csr_by(nparam, nterms, std::vector<int32_t>(t_param, t_param + nterms), t_param, t_kind, t_index,
                       t_coef, var.data());
  DevCsr d(h, c);
  static const double dummy = 0.0;
  qp_reverse_chunks(h, k, g, out_rev, [&](int s0, int64_t cols, const double* rev) {
    PhaseTimer pt(h, DOPT_PHASE_QP_OUTPUT);
    hipLaunchKernelGGL(qp_poi_reverse_k_kernel, poi_grid(nparam, cols), dim3(PTPB), 0, h.stream, rev, h.z,
                       m ? h.lam : &dummy, p ? h.nu : &dummy, n, m, p, (int)B, cols, nparam, d.ptr, d.kind, d.index,
                       d.var, d.coef, out_dp + (size_t)s0 * B * nparam);
    DOPT_CHECK_HIP(hipGetLastError());
  });
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));   // the copies out of `c` are done
}

}  // namespace

void qp_params_reverse_k(Handle& h, int k, const double* dl_dz, int nparam, int64_t nterms, const int32_t* t_param,
                         const int32_t* t_kind, const int32_t* t_index, const int32_t* t_var, const double* t_coef,
                         double* out_rev, double* out_dp) {
  qp_k_checks(h, "dopt_qp_params_reverse_k");
  if (k < 0) throw Error(-1, "dopt_qp_params_reverse_k: k must not be negative");
  validate(h, nparam, nterms, t_param, t_kind, t_index, t_coef, t_var, true);
  if (nparam == 0 || k == 0 || h.batch == 0) return;
  if (!out_dp) throw Error(-1, "dopt_qp_params_reverse_k: out_dp is required");
  if (!h.factored) qp_factor(h);
  qp_params_reverse_chunks(h, k, RevSeeds{dl_dz, nullptr, nullptr, false}, nparam, nterms, t_param, t_kind, t_index,
                           t_var, t_coef, out_rev, out_dp);
}

// Reverse with a loss gradient on the duals as well: −LHS⁻¹·[g_z; g_λ; g_ν]
// per seed (seeds with respect to the engine's λ and ν).  Every k goes through
// solve_k, so a seed's result does not depend on how the seeds are grouped.
void qp_reverse_duals_k(Handle& h, int k, const double* g_z, const double* g_lam, const double* g_nu, double* out) {
  qp_k_checks(h, "dopt_qp_reverse_duals_k");
  if (k < 1) throw Error(-1, "dopt_qp_reverse_duals_k: k must be positive");
  if (!out) throw Error(-1, "dopt_qp_reverse_duals_k: out is required");
  if (h.batch == 0) return;
  if (!h.factored) qp_factor(h);   // (also a handle that has only run the one-launch small path)
  qp_reverse_chunks(h, k, RevSeeds{g_z, g_lam, g_nu, true}, out, [](int, int64_t, const double*) {});
}

void qp_params_reverse_duals_k(Handle& h, int k, const double* g_z, const double* g_lam, const double* g_nu,
                               int nparam, int64_t nterms, const int32_t* t_param, const int32_t* t_kind,
                               const int32_t* t_index, const int32_t* t_var, const double* t_coef, double* out_rev,
                               double* out_dp) {
  qp_k_checks(h, "dopt_qp_params_reverse_duals_k");
  if (k < 1) throw Error(-1, "dopt_qp_params_reverse_duals_k: k must be positive");
  validate(h, nparam, nterms, t_param, t_kind, t_index, t_coef, t_var, true);
  if (nparam == 0 || h.batch == 0) return;
  if (!out_dp) throw Error(-1, "dopt_qp_params_reverse_duals_k: out_dp is required");
  if (!h.factored) qp_factor(h);
  qp_params_reverse_chunks(h, k, RevSeeds{g_z, g_lam, g_nu, true}, nparam, nterms, t_param, t_kind, t_index, t_var,
                           t_coef, out_rev, out_dp);
}

void conic_params_forward(Handle& h, const double* dp, int nparam, int64_t nterms, const int32_t* t_param,
                          const int32_t* t_kind, const int32_t* t_index, const double* t_coef, double* db,
                          double* dc) {
  if (!h.cset) throw Error(-1, "dopt_conic_params_forward: dopt_conic_set has not been called");
  validate_conic(h, nparam, nterms, t_param, t_kind, t_index, t_coef);
  const Csr c = conic_forward_csr(h, nterms, t_param, t_kind, t_index, t_coef);
  DevCsr d(h, c);
  {
    PhaseTimer pt(h, DOPT_PHASE_CONIC_RHS);
    launch_conic_forward(h, d, dp, 0, nparam, h.batch, db, dc);
  }
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));   // the copies out of `c` are done
}

void conic_params_reverse(Handle& h, const double* g, int nparam, int64_t nterms, const int32_t* t_param,
                          const int32_t* t_kind, const int32_t* t_index, const double* t_coef, double* out) {
  if (!h.cset) throw Error(-1, "dopt_conic_params_reverse: dopt_conic_set has not been called");
  validate_conic(h, nparam, nterms, t_param, t_kind, t_index, t_coef);
  if (nparam == 0) return;
  if (!h.cfactored) conic_factor(h);   // x and vp
  std::vector<int32_t> key(t_param, t_param + nterms);
  const Csr c = csr_by(nparam, nterms, key, t_param, t_kind, t_index, t_coef);
  DevCsr d(h, c);
  {
    PhaseTimer pt(h, DOPT_PHASE_CONIC_OUTPUT);
    launch_conic_reverse(h, d, g, nparam, h.batch, out);
  }
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));
}

// The parameter Jacobian by unit seeds, in chunks of `jacobian_chunk` seeds.
// Each chunk materialises its seeds in h.cjac — mode 0: the unit tangents
// (db_j, dc_j) = conic_params_forward(e_j) by that call's kernel; mode 1: the
// unit dx — and goes through conic_forward_k / conic_reverse_k, i.e. the
// single calls' right-hand-side kernels and the _k contract: block j is
// bit-identical to the single call on seed j whatever the chunk.  `stats`
// (host, may be null): per seed [istop | iterations], copied out of cinfok
// after each chunk.
void conic_params_jacobian(Handle& h, int mode, int nparam, int64_t nterms, const int32_t* t_param,
                           const int32_t* t_kind, const int32_t* t_index, const double* t_coef, double* out_J,
                           int32_t* stats) {
  if (!h.cset) throw Error(-1, "dopt_conic_params_jacobian: dopt_conic_set has not been called");
  if (mode != 0 && mode != 1) throw Error(-1, "dopt_conic_params_jacobian: mode must be 0 (forward) or 1 (reverse)");
  validate_conic(h, nparam, nterms, t_param, t_kind, t_index, t_coef);
  if (nparam == 0 || h.n == 0 || h.batch == 0) return;
  const size_t B = h.batch, n = h.n, m = h.m, N = n + m + 1;
  const int seeds = mode == 0 ? nparam : (int)n;
  const int chunk = jacobian_chunk(h, seeds);
  const size_t in_len = mode == 0 ? m + n : n;   // a seed's materialised input per problem
  h.cjac.ensure((size_t)chunk * B * (in_len + N) * sizeof(double));
  double* seed_in = h.cjac.as<double>();
  double* sol = seed_in + (size_t)chunk * B * in_len;
  Csr c;
  if (mode == 0) c = conic_forward_csr(h, nterms, t_param, t_kind, t_index, t_coef);
  else c = csr_by(nparam, nterms, std::vector<int32_t>(t_param, t_param + nterms), t_param, t_kind, t_index, t_coef);
  DevCsr d(h, c);
  for (int s0 = 0; s0 < seeds; s0 += chunk) {
    const int k = std::min(chunk, seeds - s0);
    const int64_t cols = (int64_t)k * (int64_t)B;
    if (mode == 0) {
      double* db = seed_in;
      double* dc = seed_in + (size_t)k * B * m;
      {
        PhaseTimer pt(h, DOPT_PHASE_CONIC_RHS);
        launch_conic_forward(h, d, nullptr, s0, nparam, cols, db, dc);
      }
      conic_forward_k(h, k, nullptr, m ? db : nullptr, dc, sol, out_J + (size_t)s0 * B * n);
    } else {
      {
        PhaseTimer pt(h, DOPT_PHASE_CONIC_RHS);
        hipLaunchKernelGGL(conic_unit_seed_kernel, poi_grid((int)n, cols), dim3(PTPB), 0, h.stream, s0, (int)n, (int)B,
                           cols, seed_in);
        DOPT_CHECK_HIP(hipGetLastError());
      }
      conic_reverse_k(h, k, seed_in, sol, nullptr, nullptr, nullptr);
      PhaseTimer pt(h, DOPT_PHASE_CONIC_OUTPUT);
      launch_conic_reverse(h, d, sol, nparam, cols, out_J + (size_t)s0 * B * nparam);
    }
    if (stats)
      DOPT_CHECK_HIP(hipMemcpyAsync(stats + (size_t)2 * B * s0, h.cinfok.p, (size_t)2 * B * k * sizeof(int32_t),
                                    hipMemcpyDeviceToHost, h.stream));
  }
  DOPT_CHECK_HIP(hipStreamSynchronize(h.stream));   // the copies out of `c` are done
}

}  // namespace dopt

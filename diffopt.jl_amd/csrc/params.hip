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
  std::vector<double> coef;
};

void validate(const Handle& h, int nparam, int64_t nterms, const int32_t* t_param, const int32_t* t_kind,
              const int32_t* t_index, const double* t_coef) {
  if (nparam < 0 || nterms < 0) throw Error(-1, "parameter accumulation: negative size");
  if (nterms > 0 && (!t_param || !t_kind || !t_index || !t_coef))
    throw Error(-1, "parameter accumulation: term arrays are required");
  for (int64_t t = 0; t < nterms; ++t) {
    const int k = t_kind[t], i = t_index[t];
    const int lim = k == 0 ? h.m : k == 1 ? h.p : k == 3 ? h.n : 1;
    if (t_param[t] < 0 || t_param[t] >= nparam || k < 0 || k > 3 || (k != 2 && (i < 0 || i >= lim)))
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
           const int32_t* t_kind, const int32_t* t_index, const double* t_coef) {
  Csr c;
  c.ptr.assign(rows + 1, 0);
  for (int64_t t = 0; t < nterms; ++t) ++c.ptr[key[t] + 1];
  std::partial_sum(c.ptr.begin(), c.ptr.end(), c.ptr.begin());
  std::vector<int64_t> pos(c.ptr.begin(), c.ptr.end() - 1);
  c.kind.resize(nterms);
  c.index.resize(nterms);
  c.param.resize(nterms);
  c.coef.resize(nterms);
  for (int64_t t = 0; t < nterms; ++t) {
    const int64_t d = pos[key[t]]++;
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
  int32_t *kind = nullptr, *index = nullptr, *param = nullptr;
  double* coef = nullptr;
  DevCsr(Handle& h, const Csr& c) {
    const hipStream_t st = h.stream;
    const size_t nt = c.coef.size(), np = c.ptr.size();
    h.pterms.ensure(np * 8 + nt * 8 + 3 * nt * 4 + 64);
    char* p = h.pterms.as<char>();
    ptr = reinterpret_cast<int64_t*>(p);
    coef = reinterpret_cast<double*>(p + np * 8);
    kind = reinterpret_cast<int32_t*>(p + np * 8 + nt * 8);
    index = kind + nt;
    param = index + nt;
    DOPT_CHECK_HIP(hipMemcpyAsync(ptr, c.ptr.data(), np * 8, hipMemcpyHostToDevice, st));
    if (nt) {
      DOPT_CHECK_HIP(hipMemcpyAsync(coef, c.coef.data(), nt * 8, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(kind, c.kind.data(), nt * 4, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(index, c.index.data(), nt * 4, hipMemcpyHostToDevice, st));
      DOPT_CHECK_HIP(hipMemcpyAsync(param, c.param.data(), nt * 4, hipMemcpyHostToDevice, st));
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

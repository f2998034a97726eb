/*
 * diffopt_mi355x.h — C ABI of the MI355X-native DiffOpt sensitivity-solve engine.
 *
 * Drop-in boundary for DiffOpt.jl's differentiation back-ends (the
 * `DiffOpt.AbstractModel` plugin layer, reference src/diff_opt.jl:274):
 *   - QuadraticProgram back-end  (src/QuadraticProgram/QuadraticProgram.jl)
 *   - ConicProgram back-end      (src/ConicProgram/ConicProgram.jl)
 * A Julia `ccall` shim (diffopt.jl_amd/julia/DiffOptMI355X.jl)
 * and the Python ctypes host (diffopt.jl_amd/diffopt_amd) bind exactly these
 * symbols.  Plain C types only: no torch/HIP types cross the boundary except an
 * opaque `void*` stream.
 *
 * Conventions
 *   - Float64 everywhere; dense arrays are COLUMN-MAJOR (Julia order) and
 *     BATCH-MAJOR: problem b's n×n `Q` starts at Q + b*n*n, its m×n `G` at
 *     G + b*m*n, its vectors at v + b*len.
 *   - QP duals are in OptNet sign (λ = −MOI dual of LessThan, ν = −MOI dual of
 *     EqualTo: QuadraticProgram.jl:164-180); the caller applies the flip.
 *   - Memory mode (dopt_set_memory): DOPT_MEM_HOST (default) — every pointer is a
 *     host pointer, inputs are copied into engine-owned HBM and outputs copied
 *     back before return.  DOPT_MEM_DEVICE — every pointer is a device pointer on
 *     the handle's device; inputs given to dopt_*_set are BORROWED (not copied)
 *     and must stay alive and unchanged until the next dopt_*_set or
 *     dopt_destroy; outputs are written in place.
 *   - Errors: return 0 on success; > 0 = LAPACK-style info of the FIRST
 *     problem whose KKT factor is exactly singular (the Julia shim raises
 *     LinearAlgebra.SingularException(info), matching `LHS \ RHS`);
 *     < 0 = argument/device error, message in dopt_last_error(h).
 *     Per-problem info: dopt_get_info().
 *   - Threading: a handle is used by one host thread at a time (the reference
 *     models are not thread-safe either).  Work runs on the handle's HIP stream;
 *     every call is synchronous at return (except a device-mode
 *     dopt_qp_forward_reverse with no singular problem: stream-ordered).
 */
#ifndef DIFFOPT_MI355X_H
#define DIFFOPT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOPT_KIND_QP 0
#define DOPT_KIND_CONIC 1
#define DOPT_KIND_NLP 2

#define DOPT_MEM_HOST 0
#define DOPT_MEM_DEVICE 1

/* cone codes for dopt_conic_set (MOI set → code); see oracle/cones.py */
#define DOPT_CONE_ZEROS 0        /* MOI.Zeros           (dual: Reals)        */
#define DOPT_CONE_NONNEG 1       /* MOI.Nonnegatives                          */
#define DOPT_CONE_NONPOS 2       /* MOI.Nonpositives                          */
#define DOPT_CONE_SOC 3          /* MOI.SecondOrderCone                       */
#define DOPT_CONE_PSD_TRI 4      /* MOI.PositiveSemidefiniteConeTriangle (side ≤ 4096; > 64 on global scratch) */

#define DOPT_ABI_VERSION 3

typedef struct dopt_handle dopt_handle;

/* Create a batched model: `batch` independent problems of identical shape.
 * QP:    n variables, m LessThan rows (G z ≤ h), p EqualTo rows (A z = b).
 * CONIC: n variables, m conic rows (A x + b ∈ K), p ignored.
 * Replaces: `MOI.instantiate(QuadraticProgram.Model)` / `ConicProgram.Model()`
 * (reference moi_wrapper.jl:605-617; QuadraticProgram.jl:107-120;
 * ConicProgram.jl:99-111).
 * A QP handle with n + m + p > 8192 takes the SPARSE route (see
 * dopt_set_sparse): no dense KKT storage is allocated. */
int dopt_create(dopt_handle** h, int device, int64_t batch, int32_t n,
                int32_t m, int32_t p, int32_t kind);
int dopt_destroy(dopt_handle* h);
const char* dopt_last_error(const dopt_handle* h);
int dopt_abi_version(void);
/* Test and diagnostic aid: the bytes of device memory that all of this
 * process's handles own at the moment (every device, staging and workspace
 * buffers included; pinned host memory, streams and events are not counted).
 * A handle's share returns to zero with dopt_destroy. */
int64_t dopt_live_device_bytes(void);
/* hipStream_t as void*; NULL = the legacy default (null) stream.  Until this
 * is called the handle uses a private non-blocking stream.  A caller that
 * produces device-mode inputs on stream S passes S here (PyTorch: the current
 * stream) so the engine's kernels are ordered after that work. */
int dopt_set_stream(dopt_handle* h, void* stream);
int dopt_set_memory(dopt_handle* h, int32_t mem);

/* ---- QuadraticProgram ------------------------------------------------------
 * Problem data + primal-dual point.  Replaces `_gradient_cache`'s inputs
 * (QuadraticProgram.jl:182-213: A, G, h, Q from MOI matrix form) and the
 * `VariablePrimalStart` / `ConstraintDualStart` setters
 * (diff_opt.jl:362-370, QuadraticProgram.jl:164-180).
 * Q: n×n Hessian (symmetrised, utils.jl:46-69); G: m×n; h: m; A: p×n;
 * z: n; lam: m; nu: p.  G/h/lam may be NULL iff m == 0; A/nu iff p == 0. */
int dopt_qp_set(dopt_handle* h, const double* Q, const double* G,
                const double* hvec, const double* A, const double* z,
                const double* lam, const double* nu);
/* Sparse route (sparse.hip; on = 1, or 2 on a conic handle).  CONIC handles: dopt_conic_set_csc keeps
 * A_moi as CSC plus a CSR copy (no dense m×n A) and every LSQR run applies M
 * matrix-free from them (ConicProgram.jl:243-247, :323, :372), one workgroup per
 * problem; PSD cones up to side 64; dopt_conic_set (dense) is refused.
 * on = DOPT_SPARSE_SPLIT (2), conic handles only: the same sparse A_moi under
 * the split LSQR — every iteration's products spread over the device (one
 * lane group per row / column of A_moi, grid of output blocks × problems), Dπ
 * one workgroup per cone, and PSD cones of any side up to dopt_create's 4096
 * (sides above 64 apply Dπ from global scratch).  The products are summed as
 * on = 1 sums them; LSQR's vector sums are the split path's, so the two modes
 * agree to LSQR's stopping noise, not bit for bit.  on = 1 stays the default
 * sparse mode; nothing picks the mode from the cone list.  Any other non-zero
 * `on` means 1.  The
 * matrix tangent and the matrix gradient have sparse forms on every conic
 * route (dopt_conic_forward_csc, dopt_conic_reverse_grads_csc below); the dense
 * dA / out_dA arguments of the other calls remain optional (NULL = skip).
 * QP handles (the sparse QP route).  The MOI matrix form stays sparse, as
 * in the reference (`_gradient_cache` keeps SparseMatrixCSC,
 * QuadraticProgram.jl:182-213): dopt_qp_set_csc keeps G and A as CSC plus a
 * CSR copy built on the device, and every solve is `lsqr(LHS, RHS)` /
 * `lsqr(LHS', RHS)` on the implicit full LHS (:486-492; IterativeSolvers 0.9
 * defaults, maxiter = n + m + p) — no dense K, no size cap.  Only the LSQR
 * branch exists on this route: dopt_qp_factor fails (−1, with a message) when
 * any problem's Q has a non-zero value (`norm(Q) ≈ 0` false, :333), since that
 * needs a sparse direct LU (UMFPACK in the reference).  Automatic for
 * n + m + p > 8192 (the dense route's cap; on = 0 is then refused); opt-in
 * below it (tests compare the two routes).  Resets the handle's model.  Not on
 * this route: dopt_qp_set (dense inputs), the multi-RHS calls, the kept mask.
 * Matrix tangents and matrix gradients at the sizes this route exists for go
 * through dopt_qp_forward_csc / dopt_qp_forward_reverse_csc /
 * dopt_qp_reverse_grads_csc (sparse tangents with their own patterns, gradients
 * sampled on a pattern); dopt_qp_forward's dense dQ / dG / dA still work here
 * (NULL = zero) for problems small enough to hold them. */
#define DOPT_SPARSE_SPLIT 2
int dopt_set_sparse(dopt_handle* h, int32_t on);
/* LSQR statistics of the sparse route's last solves, 4·B int32: per problem
 * [istop | iterations] of the reverse run, then of the forward run. */
int dopt_qp_lsqr_stats(dopt_handle* h, int32_t* stats);
/* Same as dopt_qp_set, with Q, G, A given in the MOI matrix form the
 * reference builds (`_gradient_cache`, QuadraticProgram.jl:182-213;
 * `sparse_array_representation`, utils.jl:46-69): Julia SparseMatrixCSC
 * {Float64,Int64} arrays, 1-based.  For a batch, problem b's colptr is the
 * (ncols+1) entries at X_colptr + b·(n+1) and indexes (1-based) into the
 * concatenated X_rowval / X_nzval of X_nnz entries; all three matrices have n
 * columns (Q n×n symmetrised, G m×n, A p×n).  The library densifies on the
 * device (zero fill + scatter); a malformed colptr / rowval returns −1.
 * Host mode copies the CSC arrays, device mode borrows them.  A small
 * host-mode model (its arrays packed into the handle's pinned buffer) is
 * validated on the host and the call returns with the copy and the scatter
 * queued on the handle's stream: the caller's arrays are already copied, and
 * every later call on the handle is ordered after them. */
int dopt_qp_set_csc(dopt_handle* h,
                    const int64_t* Q_colptr, const int64_t* Q_rowval, const double* Q_nzval, int64_t Q_nnz,
                    const int64_t* G_colptr, const int64_t* G_rowval, const double* G_nzval, int64_t G_nnz,
                    const int64_t* A_colptr, const int64_t* A_rowval, const double* A_nzval, int64_t A_nnz,
                    const double* hv, const double* z, const double* lam, const double* nu);
/* Assemble the KKT matrix (create_LHS_matrix, QuadraticProgram.jl:256-282),
 * select the solve branch per problem (`iterative = norm(Q) ≈ 0`, :333/:436)
 * and LU-factorise it ONCE (the reference re-factorises per call, :490).
 * Rows with λ_i == 0 and (Gz−h)_i != 0 are eliminated exactly (their
 * unknowns decouple); the rest, N' = n + kept + p rows, is factorised.
 *
 * Acceptance of a problem's no-pivot factors (else it is re-assembled and
 * factorised with partial pivoting, transparently):
 *   - threshold: every multiplier |l_ij| ≤ 10, i.e. every diagonal pivot
 *     passes UMFPACK's threshold test with tolerance 0.1;
 *   - growth: every pivot non-zero and finite, and every entry of U within
 *     1e8·max|K| (NOPIV_GROWTH, dopt_internal.h).
 * Which factorisation a problem gets:
 *   - P-symmetric route (default): when Q is exactly symmetric (checked
 *     bitwise on the device) and every kept λ is finite and non-zero, P·K is
 *     symmetric for P = diag(1, λ_k, 1), so U = D·P⁻¹·Lᵀ·P and only L is
 *     stored (U is materialised from L on demand, for single-direction and
 *     multi-RHS solves); left-looking by 64-column block columns, each
 *     diagonal block by a one-pass symmetric elimination of [P·C | I];
 *   - general no-pivot LU (right-looking, L and U stored) for the other
 *     problems of the batch;
 *   - partial pivoting for the problems either one rejects.
 * Environment switches (read at dopt_create; results agree to rounding):
 *   DOPT_LU=0    partial pivoting for every problem;
 *   DOPT_SYM=0   no P-symmetric route (the general no-pivot LU throughout);
 *   DOPT_LEFT=0  the P-symmetric problems factorised right-looking;
 *   DOPT_LDL=0   the left-looking route's diagonal blocks by the recursive
 *                32×32 LU instead of the symmetric elimination.
 * Optional: dopt_qp_reverse/forward factor on demand. */
int dopt_qp_factor(dopt_handle* h);
/* reverse_differentiate! (QuadraticProgram.jl:316-351):
 * out[b] = [dz (n) | dλ (m) | dν (p)] = −LHS \ [dl_dz; 0; 0]. */
int dopt_qp_reverse(dopt_handle* h, const double* dl_dz, double* out);
/* forward_differentiate! (QuadraticProgram.jl:357-446):
 * out[b] = [dz | dλ | dν] = −LHSᵀ \ [dQ z + dq + dGᵀλ + dAᵀν;
 *                                    λ∘(dG z) − λ∘dh; dA z − db].
 * Any tangent pointer may be NULL (= zero tangent).  dQ: n×n, dq: n,
 * dG: m×n, dh: m, dA: p×n, db: p (user tangents of Q, q, G, h, A, b — the
 * `_fill` sign handling of diff_opt.jl:594-656 is the caller's). */
int dopt_qp_forward(dopt_handle* h, const double* dQ, const double* dq,
                    const double* dG, const double* dh, const double* dA,
                    const double* db, double* out);
/* Batched reverse gradients (the reference's lazy getters, materialised for
 * every problem; QuadraticProgram.jl:448-473, :307-314, diff_opt.jl:475-481),
 * from rev = the [dz | dλ | dν] output of dopt_qp_reverse /
 * dopt_qp_forward_reverse and the handle's z, λ, ν:
 *   ReverseObjectiveFunction:  dq = dz (n),  dQ = (dz zᵀ + z dzᵀ)/2 (n×n)
 *   ReverseConstraintFunction, LessThan rows:  dG (m×n) row i = λ_i dλ_i z +
 *     λ_i dz, g_const (m) = λ_i dλ_i   (the gradient w.r.t. h is −g_const)
 *   EqualTo rows:  dA (p×n) row i = dν_i z + ν_i dz, a_const (p) = dν_i
 *     (the gradient w.r.t. b is −a_const)
 * Column-major per problem, batch-major.  Any output may be NULL. */
int dopt_qp_reverse_grads(dopt_handle* h, const double* rev, double* dQ, double* dq,
                          double* dG, double* g_const, double* dA, double* a_const);
/* k seeds / tangents per problem on one factorisation (the reference calls
 * reverse_differentiate! / forward_differentiate! once per seed on the same
 * model, re-solving each time: QuadraticProgram.jl:316-351, 357-446,
 * 486-496; callers such as docs/src/examples/sensitivity-analysis-ridge.jl:
 * 120-131 loop many seeds).  Seed-major layout: seed j's inputs are a
 * standard batch block at offset j·B·len (dl_dz: n×B×k, dq: n×B×k, dQ:
 * n×n×B×k, …), out: (n+m+p)×B×k.  Results equal k dopt_qp_reverse /
 * dopt_qp_forward calls to rounding; the blocked problems' k solves run as
 * one MFMA multi-RHS launch.  Factorises first if needed. */
int dopt_qp_reverse_k(dopt_handle* h, int32_t k, const double* dl_dz, double* out);
int dopt_qp_forward_k(dopt_handle* h, int32_t k, const double* dQ, const double* dq,
                      const double* dG, const double* dh, const double* dA,
                      const double* db, double* out);
/* Fused forward + reverse for one factorisation (the batched throughput path;
 * results identical to dopt_qp_reverse + dopt_qp_forward).  In device memory
 * mode, when every problem's factorisation is known on the host to be
 * non-singular (the no-pivot LU accepted all blocked problems), the call
 * returns once the work is queued: the outputs are stream-ordered on the
 * handle's stream (the caller's, dopt_set_stream) like any library call on
 * that stream; otherwise it returns after the singularity check. */
int dopt_qp_forward_reverse(dopt_handle* h, const double* dl_dz,
                            const double* dQ, const double* dq,
                            const double* dG, const double* dh,
                            const double* dA, const double* db,
                            double* out_rev, double* out_fwd);

/* ---- sparse tangents and on-pattern gradients (`_csc` calls) -----------------
 * The reference never densifies a matrix tangent or a matrix gradient: the
 * forward tangent is `sparse(I, J, V, rows, cols)` and enters only through
 * products (QuadraticProgram.jl:429-433; ConicProgram.jl:288-305, :314-318), and
 * the reverse gradient is a lazy rank-2 expression read at the requested
 * entries (QuadraticProgram.jl:461-473; ConicProgram.jl:430-443).  These calls do
 * the same.  A tangent matrix `X csc` is the four arguments X_colptr, X_rowval,
 * X_nzval, X_nnz in the convention of dopt_qp_set_csc: Julia
 * SparseMatrixCSC{Float64,Int64} arrays, 1-based, problem b's colptr at
 * X_colptr + b·(n+1), indexing the concatenated X_rowval / X_nzval; host mode
 * copies, device mode borrows (for the duration of the call).  A tangent has
 * ITS OWN pattern (the perturbation's, not the model's).  X_colptr == NULL: the
 * tangent is absent (zero); X_nnz == 0 with NULL rowval / nzval is valid.  A
 * pattern is colptr, rowval, nnz in the same convention.
 * Validation: a malformed colptr or rowval returns −1 with a message, as in
 * dopt_qp_set_csc; in addition the problems' entry ranges must be ascending
 * and disjoint (cp_b[1] ≥ cp_{b−1}[n+1]).  The verdict is read with the call's
 * final wait: after a −1 the outputs are unspecified, the handle's model is
 * untouched and still solves.  The staged tangents live for one call only.
 * The _k calls keep dense tangents.
 *
 * QP, sparse-route handles only (a dense-route handle returns −1 and names
 * dopt_qp_forward / dopt_qp_forward_reverse / dopt_qp_reverse_grads):
 * dopt_qp_forward with dQ (n×n), dG (m×n), dA (p×n) sparse. */
int dopt_qp_forward_csc(dopt_handle* h,
                        const int64_t* dQ_colptr, const int64_t* dQ_rowval, const double* dQ_nzval, int64_t dQ_nnz,
                        const double* dq,
                        const int64_t* dG_colptr, const int64_t* dG_rowval, const double* dG_nzval, int64_t dG_nnz,
                        const double* dh,
                        const int64_t* dA_colptr, const int64_t* dA_rowval, const double* dA_nzval, int64_t dA_nnz,
                        const double* db, double* out);
/* dopt_qp_forward_reverse with sparse dQ, dG, dA. */
int dopt_qp_forward_reverse_csc(dopt_handle* h, const double* dl_dz,
                                const int64_t* dQ_colptr, const int64_t* dQ_rowval, const double* dQ_nzval,
                                int64_t dQ_nnz, const double* dq,
                                const int64_t* dG_colptr, const int64_t* dG_rowval, const double* dG_nzval,
                                int64_t dG_nnz, const double* dh,
                                const int64_t* dA_colptr, const int64_t* dA_rowval, const double* dA_nzval,
                                int64_t dA_nnz, const double* db, double* out_rev, double* out_fwd);
/* dopt_qp_reverse_grads' matrix gradients read at the entries of a pattern:
 * out_dX_nz[k] for entry k = (i, j) of problem b, in the pattern's order,
 *   dQ_ij = (dz_i z_j + z_i dz_j)/2,  dG_ij = λ_i dλ_i z_j + λ_i dz_j,
 *   dA_ij = dν_i z_j + ν_i dz_j.
 * An output that is NULL is skipped.  A NULL G / A colptr with a non-NULL
 * output means the pattern the handle got from dopt_qp_set_csc (out of G_nnz /
 * A_nnz entries); Q's pattern is not kept and must be given.  An entry index no
 * problem's column range covers is left untouched. */
int dopt_qp_reverse_grads_csc(dopt_handle* h, const double* rev,
                              const int64_t* Q_colptr, const int64_t* Q_rowval, int64_t Q_nnz, double* out_dQ_nz,
                              const int64_t* G_colptr, const int64_t* G_rowval, int64_t G_nnz, double* out_dG_nz,
                              const int64_t* A_colptr, const int64_t* A_rowval, int64_t A_nnz, double* out_dA_nz);

/* ---- parameters (ParametricOptInterface glue, reference src/parameters.jl) ----
 * A parametric term t: t_param[t] ∈ [0, nparam), t_kind[t]:
 *   0  parameter term of LessThan row t_index[t]   (ParametricAffineFunction)
 *   1  parameter term of EqualTo row t_index[t]
 *   2  parameter term of the objective (t_index ignored)
 *   3  parameter×variable term of the objective, variable t_index[t]
 * and coefficient t_coef[t]; identical for every problem of the batch.  Term
 * arrays are host memory in both memory modes; sums run in term order.
 * Reverse (parameters.jl:341-534, reverse_differentiate! of POI.Optimizer):
 * out_dp (nparam×B) = Σ_t c_t·s_t from a reverse output rev ((n+m+p)×B):
 * s = λ_i·dλ_i (kind 0, the constant of ReverseConstraintFunction), dν_i
 * (kind 1), 0 (kind 2, ReverseObjectiveFunction's constant), dz_v (kind 3, its
 * coefficient of v) — ReverseConstraintSet of each parameter.
 * Forward (parameters.jl:91-300, forward_differentiate! of POI.Optimizer):
 * from parameter tangents dp (nparam×B), the constraint / objective tangents
 * in dopt_qp_forward's inputs: dh_i = −Σ c·dp (LessThan constants, the
 * `_fill` negation), db_i = −Σ c·dp (EqualTo), dq_v = Σ c·dp (kind 3);
 * kind 2 does not enter the KKT system. */
int dopt_qp_params_reverse(dopt_handle* h, const double* rev, int32_t nparam, int64_t nterms,
                           const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                           const double* t_coef, double* out_dp);
int dopt_qp_params_forward(dopt_handle* h, const double* dp, int32_t nparam, int64_t nterms,
                           const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                           const double* t_coef, double* dq, double* dh, double* db);
/* The parameter calls on k seeds, solves included (the `_k` contract above:
 * seed-major blocks, one factorisation, dense-route handles only, the return
 * value is the first singular problem's info).  Two more term kinds, the
 * parameter×variable terms c·p·x_v of a ParametricQuadraticFunction constraint
 * (parameters.jl:147-203 forward, :390-441 reverse):
 *   4  of LessThan row t_index[t] ∈ [0, m), variable t_var[t] ∈ [0, n)
 *   5  of EqualTo row t_index[t] ∈ [0, p), variable t_var[t]
 * t_var may be NULL when no term has kind 4 or 5 and is ignored for kinds 0-3.
 * dopt_qp_params_forward / dopt_qp_params_reverse above keep refusing kinds 4
 * and 5 ("out of range"): they have no dG / dA to write such a term to.
 * Parameter×parameter terms (parameters.jl:161-178) multiply by the VALUE of
 * the other parameter, which differs per problem while a coefficient here is
 * shared by the batch: the caller folds them into kind 0, 1 or 2 terms per
 * batch of equal values.
 * dopt_qp_params_forward_k: dp nparam×B×k (k blocks in dopt_qp_params_forward's
 * layout), out (n+m+p)×B×k as dopt_qp_forward_k's.  Seed j's block equals, to
 * rounding, dopt_qp_forward on the tangents the terms define — dq_v = Σ c·dp
 * (kind 3), dh_i = −Σ c·dp (kind 0), db_i = −Σ c·dp (kind 1), dG[i,v] = Σ c·dp
 * (kind 4), dA[i,v] = Σ c·dp (kind 5), kind 2 dropped — but the right-hand
 * sides are written straight from the term table: no dense tangent is formed.
 * dp == NULL: unit seeds, k must equal nparam (else −1), seed j is e_j — the
 * forward-mode Jacobian: block j = [dz/dp_j; dλ/dp_j; dν/dp_j].
 * dopt_qp_params_reverse_k: dl_dz n×B×k as dopt_qp_reverse_k's, out_rev
 * (n+m+p)×B×k (may be NULL), out_dp nparam×B×k = Σ_t c_t·s_t with s the getter
 * the reference reads: kinds 0-3 as dopt_qp_params_reverse, kind 4
 * λ_i·dλ_i·z_v + λ_i·dz_v, kind 5 dν_i·z_v + ν_i·dz_v (the dG / dA entries of
 * dopt_qp_reverse_grads).  dl_dz == NULL: unit seeds, k must equal n, seed i is
 * e_i — the reverse-mode Jacobian: block i is row i of dz/dp.
 * nparam == 0, k == 0 or batch == 0: nothing is written, 0 is returned; k < 0
 * returns −1.  A seed's block does not depend on how the seeds are grouped
 * (chunks of a multiple of 16 seeds within 1 GiB of work vectors; the
 * environment variable DOPT_QP_JAC_CHUNK=<k ≥ 1> overrides the chunk). */
int dopt_qp_params_forward_k(dopt_handle* h, int32_t k, const double* dp, int32_t nparam, int64_t nterms,
                             const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                             const int32_t* t_var, const double* t_coef, double* out);
int dopt_qp_params_reverse_k(dopt_handle* h, int32_t k, const double* dl_dz, int32_t nparam, int64_t nterms,
                             const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                             const int32_t* t_var, const double* t_coef, double* out_rev, double* out_dp);
/* Reverse mode with a loss gradient on the duals as well: for a loss
 * l(z, λ, ν), per seed and problem
 *   [dz; dλ; dν] = −LHS⁻¹ · [dl/dz; dl/dλ; dl/dν]
 * with LHS = [Q, GᵀD(λ), Aᵀ; G, D(Gz−h), 0; A, 0, 0] as dopt_qp_reverse solves
 * it with [dl/dz; 0; 0]; an eliminated inequality row (λ_i == 0, s_i ≠ 0)
 * recovers as x_λi = (dl/dλ_i − G_i·x_z)/s_i.  The output feeds the same
 * getters (dopt_qp_reverse_grads, dopt_qp_params_reverse): dq = dz, g_const_i =
 * λ_i·dλ_i, …  Sign convention: the seeds are with respect to the engine's λ
 * and ν (the OptNet sign dopt_qp_set takes), which are minus the MOI duals — a
 * caller holding dl/d(MOI dual) passes its negative.  The reference's QP
 * back-end ignores ReverseConstraintDual (QuadraticProgram.jl:329 solves with
 * [dl_dz; 0; 0]; moi_wrapper.jl:532-533 forwards the attribute, diff_opt.jl:
 * 396-402 stores it, the NLP back-end reads it): this is the engine's extension
 * of it, with the same getters as the reference.
 * dl_dz n×B×k, dl_dlam m×B×k, dl_dnu p×B×k, seed-major as every _k call; each
 * may be NULL (= 0) but not all three (−1: there is no unit-seed mode here);
 * dl_dlam is ignored when m == 0, dl_dnu when p == 0.  out (n+m+p)×B×k =
 * [dz | dλ | dν].  k ≥ 1, every k through the multi-RHS solve: a seed's block
 * does not depend on how the seeds are grouped (chunks as the parameter _k
 * calls, DOPT_QP_JAC_CHUNK included), and with zero dual seeds it is
 * dopt_qp_reverse_k's (k ≥ 2) bit for bit.  Factorises first if needed; returns
 * the first singular problem's info.  On the sparse route: k == 1 only (LSQR on
 * the full LHS), no singular verdict.
 * dopt_qp_params_reverse_duals_k: the same solve, then the accumulation of
 * dopt_qp_params_reverse_k (kinds 0-5; out_rev may be NULL); dense-route
 * handles only. */
int dopt_qp_reverse_duals_k(dopt_handle* h, int32_t k, const double* dl_dz, const double* dl_dlam,
                            const double* dl_dnu, double* out);
int dopt_qp_params_reverse_duals_k(dopt_handle* h, int32_t k, const double* dl_dz, const double* dl_dlam,
                                   const double* dl_dnu, int32_t nparam, int64_t nterms, const int32_t* t_param,
                                   const int32_t* t_kind, const int32_t* t_index, const int32_t* t_var,
                                   const double* t_coef, double* out_rev, double* out_dp);

/* ---- ConicProgram ----------------------------------------------------------
 * A: m×n MOI coefficients (A_moi x + b ∈ K; the diffcp sign flip of
 * ConicProgram.jl:179-183 is applied inside), b: m MOI constants, c: n
 * objective (already negated by the caller for MAX_SENSE, :206-208),
 * x: n, s: m (ConstraintPrimalStart), y: m (ConstraintDualStart).
 * cone_desc: 2*ncones int32 pairs (code, dimension) in row order (the
 * ProductOfSets layout, product_of_sets.jl:15-74); identical for every
 * problem of the batch. */
int dopt_conic_set(dopt_handle* h, const double* A, const double* b,
                   const double* c, const double* x, const double* s,
                   const double* y, const int32_t* cone_desc, int32_t ncones);
/* dopt_conic_set with A_moi in the reference's MOI matrix form (ConicProgram.jl
 * _gradient_cache :172-255 reads it from MatrixOfConstraints): Julia
 * SparseMatrixCSC{Float64,Int64} arrays, 1-based, batch layout as in
 * dopt_qp_set_csc (colptr at offset b·(n+1), indexes into the concatenated
 * rowval / nzval); densified on the device, malformed indices return −1. */
int dopt_conic_set_csc(dopt_handle* h, const int64_t* A_colptr, const int64_t* A_rowval,
                       const double* A_nzval, int64_t A_nnz, const double* b, const double* c,
                       const double* x, const double* s, const double* y,
                       const int32_t* cone_desc, int32_t ncones);
/* _gradient_cache (ConicProgram.jl:172-255): v = y − s, Dπ(v), π(v), M.
 * Returns −1 with the reference's message ("Some constraints are missing a
 * value for the `ConstraintDualStart` attribute." / `ConstraintPrimalStart`,
 * ConicProgram.jl:186-196) when some y or s entry is NaN (the reference's
 * marker of a missing start). */
int dopt_conic_factor(dopt_handle* h);
/* forward_differentiate! (ConicProgram.jl:257-334): out[b] = [du | dv | dw]
 * (n+m+1) = lsqr(M, [dAᵀvp + dc; −dA x + db; −dc·x − db·vp]) (0 if the RHS is
 * exactly zero, :320).  out_dx (optional, n per problem) receives
 * ForwardVariablePrimal = −(du − x·dw) (:403-412).  dA/db/dc may be NULL. */
int dopt_conic_forward(dopt_handle* h, const double* dA, const double* db,
                       const double* dc, double* out, double* out_dx);
/* reverse_differentiate! (ConicProgram.jl:336-394), dy = ds = 0:
 * out_g[b] = lsqr(M, [dx; 0; −xᵀdx]) (0 if its norm ≤ 1e-4, :369-370).
 * Optional outputs (any may be NULL): out_dA (m×n col-major) =
 * g_v xᵀ − vp g_xᵀ, out_db (m) = g_v − g_end·vp, out_dc (n) = g_x − g_end·x
 * (getters :396-443). */
int dopt_conic_reverse(dopt_handle* h, const double* dx, double* out_g,
                       double* out_dA, double* out_db, double* out_dc);
/* forward_differentiate! and reverse_differentiate! of every problem in one
 * call (the bench step): both LSQR runs co-iterated in one kernel, sharing
 * each sweep over A (ConicProgram.jl:323, :372; per-direction stopping rules
 * kept), outputs as dopt_conic_forward (out, out_dx) and dopt_conic_reverse
 * (out_g, out_dA, out_db, out_dc; any of out_dx / out_dA / out_db / out_dc
 * may be NULL).  Bit-identical to the two separate calls. */
int dopt_conic_forward_reverse(dopt_handle* h, const double* dA, const double* db,
                               const double* dc, const double* dx, double* out,
                               double* out_dx, double* out_g, double* out_dA,
                               double* out_db, double* out_dc);
/* The `_csc` forms (conventions above, at dopt_qp_forward_csc), on EVERY conic
 * route — the right-hand side does not depend on how LSQR runs.
 * dopt_conic_forward with dA (m×n) as a sparse tangent with its own pattern:
 * the right-hand side takes dAᵀvp and dA·x from the tangent's CSC / CSR copies,
 * never from a dense m×n array.  A NULL colptr or an empty tangent gives
 * dopt_conic_forward(dA = NULL)'s result bit for bit. */
int dopt_conic_forward_csc(dopt_handle* h, const int64_t* dA_colptr, const int64_t* dA_rowval,
                           const double* dA_nzval, int64_t dA_nnz, const double* db, const double* dc,
                           double* out, double* out_dx);
/* dopt_conic_forward_reverse with the sparse tangent; no dense out_dA (read
 * the gradient with dopt_conic_reverse_grads_csc).  Bit-identical to
 * dopt_conic_forward_csc plus dopt_conic_reverse. */
int dopt_conic_forward_reverse_csc(dopt_handle* h, const int64_t* dA_colptr, const int64_t* dA_rowval,
                                   const double* dA_nzval, int64_t dA_nnz, const double* db, const double* dc,
                                   const double* dx, double* out, double* out_dx, double* out_g,
                                   double* out_db, double* out_dc);
/* The reverse gradient dA read at the entries of a pattern (`_get_dA`,
 * ConicProgram.jl:430-443): g = a reverse call's out_g ((n+m+1)×B);
 * out_nz[k] = g[n+i]·x[j] − vp[i]·g[j] for entry k = (i, j) of problem b, in the
 * pattern's order; an entry index no problem's column range covers is left
 * untouched.  Needs a factored handle (x, vp).  P_colptr == NULL: the pattern
 * the handle got from dopt_conic_set_csc (out_nz of A_nnz entries) — sparse-route
 * handles only, where it is kept; elsewhere −1. */
int dopt_conic_reverse_grads_csc(dopt_handle* h, const double* g, const int64_t* P_colptr,
                                 const int64_t* P_rowval, int64_t P_nnz, double* out_nz);
/* Caps LSQR at `maxiter` iterations (0 restores the reference's default,
 * IterativeSolvers' maxiter = max(size(M)) = n + m + 1: ConicProgram.jl:323,
 * :372); a run that reaches the cap reports istop 7.  A parity instrument:
 * on an ill-conditioned M, where the converged outputs depend on rounding,
 * the iterates at a fixed small k are still comparable to 1e-6. */
int dopt_conic_set_maxiter(dopt_handle* h, int32_t maxiter);
/* LSQR statistics of the last conic call, 4·B int32: [istop | iterations] of
 * the last (or, after dopt_conic_forward_reverse, the reverse) run, then
 * [istop | iterations] of the forward run of dopt_conic_forward_reverse. */
int dopt_conic_lsqr_stats(dopt_handle* h, int32_t* stats);
/* LSQR's terminal scalar estimates of the same runs, 8·B doubles: per problem
 * (rnorm, arnorm, xnorm, anorm) — ‖b − Mx‖, ‖Mᵀ(b − Mx)‖, ‖x‖ and the
 * Frobenius estimate of ‖M‖ as IterativeSolvers' lsqr accumulates them at its
 * last iteration (0 for a zero right-hand side) — of the last (or reverse)
 * run, then of the forward run of dopt_conic_forward_reverse.  Test/bench
 * introspection (no reference counterpart: lsqr's log is not kept,
 * ConicProgram.jl:323, :372). */
int dopt_conic_lsqr_norms(dopt_handle* h, double* norms);
/* k seeds per solved cone program in one call: k reverse_differentiate!
 * (ConicProgram.jl:336-394, getters :396-443) or k forward_differentiate!
 * (:257-334) of every problem, where the reference re-runs lsqr(M, ·) once per
 * seed (:323, :372).  Seed-major layout as dopt_qp_reverse_k: seed j's inputs
 * and outputs are an ordinary batch block at offset j·B·len (dx n×B×k, out_g
 * (n+m+1)×B×k, out_dA m×n×B×k col-major per problem, …).  The same pointers
 * may be NULL as in dopt_conic_reverse / dopt_conic_forward; k >= 1 (else −1);
 * factorises first if needed.  Seed j's outputs, istop and iteration count are
 * bit-identical to the single-seed call on that seed alone, on every route —
 * the per-seed special cases (a reverse seed with ‖dz‖ ≤ 1e-4 → 0, :369-370;
 * a forward seed with an exactly zero RHS → 0, :320) and
 * dopt_conic_set_maxiter included.  Dense persistent route (m ≤ 1024, PSD
 * sides ≤ 64, not dopt_set_sparse): groups of up to 4 seeds co-iterate in one
 * workgroup and share every sweep over A (k = 1: the single-seed kernel).
 * Split route and sparse route: the single-seed LSQR once per seed inside the
 * call — no shared sweep there yet.  The _k calls keep dense tangents and a
 * dense out_dA (no `_csc` form).
 * After a _k call dopt_conic_lsqr_stats, dopt_conic_lsqr_norms, dopt_get_info
 * and dopt_get_system_size report seed 0. */
int dopt_conic_reverse_k(dopt_handle* h, int32_t k, const double* dx, double* out_g,
                         double* out_dA, double* out_db, double* out_dc);
int dopt_conic_forward_k(dopt_handle* h, int32_t k, const double* dA, const double* db,
                         const double* dc, double* out, double* out_dx);
/* LSQR statistics of the last _k call, 2·B·k int32: per seed [istop (B) |
 * iterations (B)].  −1 if the last conic call was not a _k call with this k. */
int dopt_conic_lsqr_stats_k(dopt_handle* h, int32_t k, int32_t* stats);

/* ---- parameters of a cone program (reference src/parameters.jl:341-534
 * consuming ConicProgram.jl:396-443; test/parameters.jl:103-152) -------------
 * Terms as dopt_qp_params_*: (t_param, t_kind, t_index, t_coef), host memory in
 * both memory modes, identical for every problem, sums in term order.  Kinds
 * keep the QP numbers where they mean the same thing:
 *   0  parameter term of constraint row t_index ∈ [0, m), ProductOfSets row
 *      order (ParametricVectorAffineFunction; the caller maps output_index to
 *      the row)
 *   2  parameter term of the objective (t_index ignored)
 *   3  parameter×variable term of the objective, variable t_index ∈ [0, n)
 * kind 1 and anything else is refused (−1, "parameter accumulation: term T out
 * of range").
 * Forward (parameters.jl:120-145, :226-275, then ConicProgram.jl:270-287):
 * from dp (nparam×B), dopt_conic_forward's inputs db (m×B) and dc (n×B),
 * written in full: db_i = +Σ c·dp over row i's kind-0 terms — no negation:
 * the conic `_fill` runs with S -> false, unlike the QP's dh / db —, dc_v =
 * Σ c·dp over kind 3; kind 2 is dropped.
 * Reverse (parameters.jl:365-388, :463-509): out_dp (nparam×B) = Σ_t c_t·s_t
 * from a reverse call's out_g ((n+m+1)×B): s = the value dopt_conic_reverse
 * writes to out_db[i], g[n+i] − g[n+m]·vp[i] (kind 0), to out_dc[v],
 * g[v] − g[n+m]·x[v] (kind 3), 0 (kind 2: ReverseObjectiveFunction's constant
 * is 0.0, ConicProgram.jl:400).  Needs x and vp: factorises first if needed.
 * The two directions are NOT adjoint: reverse_differentiate! runs lsqr on M,
 * not Mᵀ (ConicProgram.jl:372, TODO :381-384), and M is singular at every
 * exact primal-dual point. */
int dopt_conic_params_forward(dopt_handle* h, const double* dp, int32_t nparam, int64_t nterms,
                              const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                              const double* t_coef, double* db, double* dc);
int dopt_conic_params_reverse(dopt_handle* h, const double* g, int32_t nparam, int64_t nterms,
                              const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                              const double* t_coef, double* out_dp);
/* The parameter Jacobian by unit seeds; each direction restates its k
 * reference calls (they are different objects, see above: there is no mode that
 * picks one for the caller).  mode 0: out_J is n×B×nparam, seed-major as every
 * _k output: block j = the out_dx of dopt_conic_forward(NULL, db_j, dc_j) with
 * (db_j, dc_j) = dopt_conic_params_forward(e_j) (ForwardConstraintSet of
 * parameter j = 1, forward_differentiate!, ForwardVariablePrimal).  mode 1:
 * out_J is nparam×B×n: block i = dopt_conic_params_reverse of the out_g of
 * dopt_conic_reverse(dx = e_i) (ReverseVariablePrimal of variable i = 1,
 * reverse_differentiate!, ReverseConstraintSet of every parameter).  Any
 * other mode: −1.  The seeds run through dopt_conic_forward_k / _reverse_k in
 * chunks (sized from a workspace bound; env DOPT_CONIC_JAC_CHUNK=<k> overrides)
 * and every block is bit-identical to those single calls on its seed, whatever
 * the chunk.  A parameter whose terms never enter (none, or kind 2 only) has
 * an exactly zero right-hand side: its mode-0 block is 0 with istop 0
 * (ConicProgram.jl:320).  stats (host memory, may be NULL): 2·B·K int32, K =
 * nparam (mode 0) or n (mode 1), laid out as dopt_conic_lsqr_stats_k.  nparam =
 * 0 or n = 0 writes nothing and returns 0.  After the call
 * dopt_conic_lsqr_stats_k returns −1. */
int dopt_conic_params_jacobian(dopt_handle* h, int32_t mode, int32_t nparam, int64_t nterms,
                               const int32_t* t_param, const int32_t* t_kind, const int32_t* t_index,
                               const double* t_coef, double* out_J, int32_t* stats);

/* ---- introspection ---------------------------------------------------------*/
/* per-problem status of the last factor/solve: QP: 0 ok, k>0 zero pivot at
 * column k of the reference's KKT matrix LHS (unknowns [z; λ; ν], 1-based;
 * the engine factorises the reduced system and maps its column back);
 * CONIC: LSQR istop of the last solve. */
/* ---- NonLinearProgram back-end (kind DOPT_KIND_NLP) ------------------------
 * dopt_create's n = primal variables, m = NLP constraints c, p = parameters P.
 * Replaces the KKT part of src/NonLinearProgram (the derivatives at the
 * solution are evaluated by the caller, as the reference's MOI Nonlinear
 * evaluator does, nlp_utilities.jl:35-92):
 *   _compute_solution_and_bounds + _build_sensitivity_matrices
 *     (nlp_utilities.jl:181-396)                  -> dopt_nlp_set_structure / _set
 *   _lu_with_inertia_correction (NonLinearProgram.jl:394-422) -> dopt_nlp_factor
 *   forward_differentiate! (NonLinearProgram.jl:502-528)       -> dopt_nlp_forward
 *   reverse_differentiate! (NonLinearProgram.jl:530-582)       -> dopt_nlp_reverse
 *   _compute_sensitivity's ∂s (nlp_utilities.jl:457-500)      -> dopt_nlp_jacobian
 * Every array is batch-major; matrices are column-major per problem (Julia
 * layout, as the QP entry points). */
/* con_kind[c]: 0 EqualTo, 1 GreaterThan, 2 LessThan, in NLP constraint order;
 * has_low / has_up[n]: VariableIndex-in-GreaterThan / LessThan bounds;
 * sense: +1 MIN_SENSE, -1 MAX_SENSE.  Shared by the batch. */
int dopt_nlp_set_structure(dopt_handle* h, const int32_t* con_kind, const int8_t* has_low,
                           const int8_t* has_up, int32_t sense);
/* Hxx[n×n], Hxp[n×P]: Hessian of f − sense·yᵀc (eval_hessian_lagrangian with
 * σ = 1, μ = −sense·y) over primal × primal / primal × parameter;
 * Jx[c×n], Jp[c×P]: constraint Jacobian; x[n]; cval[c] = c(x) and crhs[c] the
 * set constant (slack = cval − crhs); y[c], yl[n], yu[n]: MOI ConstraintDual
 * values of the rows and of the bounds; xl[n], xu[n]: bound values (entries of
 * unbounded variables are ignored; yl/yu/xl/xu may be NULL when no variable
 * has that bound). */
int dopt_nlp_set(dopt_handle* h, const double* Hxx, const double* Hxp, const double* Jx,
                 const double* Jp, const double* x, const double* cval, const double* crhs,
                 const double* y, const double* xl, const double* xu, const double* yl,
                 const double* yu);
/* LU of every problem's M with the reference's inertia correction
 * (M + k·1e-6·D, k ≤ 50); a problem whose correction fails gets ∂s = 0, as
 * in the reference (nlp_utilities.jl:436-439).  Synchronous at return by
 * default: every verdict (fallbacks, corrections, the factorisation of a
 * missed speculative launch — below) is final when the call returns.  On the
 * reduced route the LU is launched without reading the sizes back first, on
 * the guess that every problem is reduced and H symmetric; the call redoes the
 * factorisation when the guess missed (the handle then stops guessing until the
 * next dopt_nlp_set_structure). */
int dopt_nlp_factor(dopt_handle* h);
/* Opt-in (on = 1): dopt_nlp_factor returns once the LU is QUEUED, and the
 * next call that needs the factors (forward / reverse / forward_reverse /
 * jacobian / kkt_solve / get_corrections / get_system_size / get_lu_kind)
 * reads the verdicts back, overlapping that wait with its own right-hand sides
 * (config 6: ≈ 3 % per step).  The price: until that next call the handle
 * still needs its inputs — in device mode they must stay unchanged (a
 * fallback or a missed speculative launch re-reads them; a change in between
 * gives undefined results), and an argument error of the factorisation
 * surfaces from that next call.  Host mode copies the inputs, so only the
 * error timing differs there.  on = 0 finishes a pending factorisation. */
int dopt_nlp_set_deferred(dopt_handle* h, int32_t on);
/* dp[P] → dx[n], ddual[c + nlow + nup] (constraint duals, then the duals of
 * the primal lower and upper bounds in variable order): ∂s·Δp. */
int dopt_nlp_forward(dopt_handle* h, const double* dp, double* dx, double* ddual);
/* dx[n], ddual[c + nlow + nup] (either may be NULL = 0) → dp[P] = ∂sᵀΔw. */
int dopt_nlp_reverse(dopt_handle* h, const double* dx, const double* ddual, double* dp);
/* Both of the above against the same factors in one call (forward_differentiate!
 * then reverse_differentiate!, NonLinearProgram.jl:502-582): dp → dx_out,
 * ddual_out and dx_seed, ddual_seed (either may be NULL = 0) → dp_out; one
 * pass over the factors serves both directions.  Results equal
 * dopt_nlp_forward + dopt_nlp_reverse. */
int dopt_nlp_forward_reverse(dopt_handle* h, const double* dp, const double* dx_seed,
                             const double* ddual_seed, double* dx_out, double* ddual_out,
                             double* dp_out);
/* ∂s itself: ds[rows × P] per problem (column-major), rows = the size of M
 * (dopt_nlp_get_layout). */
int dopt_nlp_jacobian(dopt_handle* h, double* ds);
/* corrections applied per problem (0 none, k > 0, -1 failed) */
int dopt_nlp_get_corrections(dopt_handle* h, int32_t* corr);
/* layout[7] = {rows, num_w, c, nlo, nup, nlow_primal, nup_primal} */
int dopt_nlp_get_layout(dopt_handle* h, int32_t* layout);
/* KKT mode — the reference's NonLinearKKTJacobianFactorization plug point
 * (`(M, model) -> K`, then ldiv!(∂s, K, N), nlp_utilities.jl:436-442): M[rows ×
 * rows] per problem, num_w / num_cons set the inertia correction's D.  Then
 * dopt_nlp_factor and dopt_nlp_kkt_solve: x = K \ rhs for k right-hand sides
 * per problem, rhs / x seed-major (k × batch × rows). */
int dopt_nlp_set_kkt(dopt_handle* h, int32_t rows, int32_t num_w, int32_t num_cons, const double* M);
int dopt_nlp_kkt_solve(dopt_handle* h, int32_t k, const double* rhs, double* x);
/* The reference's narrow QP plug point, QuadraticProgram.LinearAlgebraSolver
 * (QuadraticProgram.jl:475-502; exercised at test/moi_wrapper.jl:74-98):
 * solve_system(solver, LHS, RHS, iterative) = iterative ? lsqr(LHS, RHS) :
 * LHS \ RHS, for a given square matrix per problem — the reference passes its
 * assembled KKT LHS for reverse and LHS' for forward (:335, :438).  On a
 * DOPT_KIND_NLP handle: M column-major rows × rows × batch, k right-hand sides
 * seed-major (k × batch × rows), x the same shape.  LU: the blocked LU
 * without inertia correction; returns > 0 (a zero-pivot column, 1-based) for
 * a singular LHS — the Julia shim raises SingularException as `\` does.
 * iterative: LSQR with IterativeSolvers' defaults, as the reference. */
int dopt_lhs_solve(dopt_handle* h, int32_t rows, const double* M, int32_t k, const double* rhs, double* x,
                   int32_t iterative);
/* A further solve on the factorisation of the last non-iterative
 * dopt_lhs_solve of this handle: M x = rhs (trans 0) or Mᵀ x = rhs (trans 1),
 * same shapes; returns that call's info again (Mᵀ is singular exactly when M
 * is).  The plug point's second call per model (`LHS'`, QuadraticProgram.jl:438,
 * after `LHS` at :335) then costs the solves, not a second factorisation —
 * the Julia shim takes it when the adjoint's parent is the matrix it last
 * factorised.  < 0 if no such factorisation is held. */
int dopt_lhs_resolve(dopt_handle* h, int32_t k, const double* rhs, double* x, int32_t trans);

int dopt_get_info(dopt_handle* h, int32_t* info);
/* per-problem `iterative` branch flags (QP; 1 = LSQR branch). */
int dopt_get_iterative(dopt_handle* h, int8_t* flags);
/* QP kept-row mask of the last factorisation: kept[b·m + i] = 1 if
 * inequality row i of problem b stays in the factorised system, 0 if it was
 * eliminated exactly (λ_i == 0 and (Gz − h)_i != 0, with Gz − h summed in
 * Julia's sparse mul! order) — the bit-exact discrete selection. */
int dopt_qp_get_kept(dopt_handle* h, int8_t* kept);
/* QP factorisation kind per problem of the last factorisation. */
#define DOPT_LU_KIND_LSQR 0      /* `iterative` branch (no factorisation)        */
#define DOPT_LU_KIND_NOPIV 1     /* no-pivot LU passed the threshold test        */
#define DOPT_LU_KIND_PIVOT 2     /* partial pivoting                             */
#define DOPT_LU_KIND_SMALL 3     /* no-pivot LU of the one-workgroup small path  */
int dopt_qp_get_lu_kind(dopt_handle* h, int8_t* kinds);
/* per-problem flag: 1 when the last factorisation took the P-symmetric
 * no-pivot route (P = diag(1, λ_k, 1) makes P·K symmetric: lower trailing
 * tiles only, U from L, ≈ N'³/3 flops instead of 2N'³/3), 0 otherwise.
 * On a sparse-route handle (dopt_set_sparse) nothing is factorised: every
 * flag is 0, whatever an earlier dense factorisation on the handle took.
 * Introspection for tests and the bench. */
int dopt_qp_get_sym(dopt_handle* h, int8_t* flags);
/* per-problem size of the factorised (reduced) KKT system (QP; NLP: n + c on
 * the reduced route, the rows of M on the full one) or LSQR iteration count
 * of the last solve (CONIC). */
int dopt_get_system_size(dopt_handle* h, int32_t* sizes);
/* Per-phase GPU time, measured with HIP events on the handle's stream around
 * each phase's kernels while profiling is on (off by default). */
#define DOPT_PHASE_QP_ASSEMBLE 0  /* branch flag, s = Gz − h, elimination, KKT   */
#define DOPT_PHASE_QP_LU 1        /* no-pivot blocked LU                         */
#define DOPT_PHASE_QP_LU_PIVOT 2  /* partial-pivoting LU (rejected problems, the
                                     generic unblocked LU, NLP factorisations)  */
#define DOPT_PHASE_QP_RHS 3       /* forward/reverse right-hand sides            */
#define DOPT_PHASE_QP_SOLVE 4     /* triangular solves                           */
#define DOPT_PHASE_QP_LSQR 5      /* LSQR (norm(Q) == 0 branch)                  */
#define DOPT_PHASE_QP_OUTPUT 6    /* output recovery / scatter                   */
#define DOPT_PHASE_CONIC_CONE 7   /* π(v), Dπ(v) per cone                        */
#define DOPT_PHASE_CONIC_RHS 8    /* conic right-hand sides                      */
#define DOPT_PHASE_CONIC_LSQR 9   /* conic LSQR on M                             */
#define DOPT_PHASE_CONIC_OUTPUT 10
#define DOPT_NUM_PHASES 11
int dopt_set_profiling(dopt_handle* h, int32_t on);
/* Profiling restricted to the phases in `mask` (bit DOPT_PHASE_x; 0 = off).
 * The events of a timed phase cost a few microseconds of queue time each, so
 * a benchmark times only the phase it reports live and takes the breakdown
 * of the others from a separate pass. */
int dopt_set_profiling_phases(dopt_handle* h, uint32_t mask);
/* Accumulated milliseconds and launch counts per phase since the last call
 * (arrays of length nphases ≤ DOPT_NUM_PHASES); resets the accumulators. */
int dopt_get_phase_times(dopt_handle* h, double* ms, int32_t* counts,
                         int32_t nphases);
const char* dopt_phase_name(int32_t phase);
/* wall time (s) of the last forward/reverse call, incl. any factorisation it
 * triggered — the DifferentiateTimeSec analogue (diff_opt.jl:256-266).
 * Exception: a device-mode dopt_qp_forward_reverse that returned
 * stream-ordered (see above) records only the time to queue its work; call
 * hipStreamSynchronize on the handle's stream and time around it for the
 * completed solve. */
double dopt_last_time(const dopt_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* DIFFOPT_MI355X_H */

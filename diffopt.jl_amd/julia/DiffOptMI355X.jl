# DiffOptMI355X.jl — Julia side of the drop-in boundary (INTEGRATION.md).
#
# Two `DiffOpt.AbstractModel` back-ends (the plug point of reference
# src/diff_opt.jl:274, selected with `MOI.set(model, DiffOpt.ModelConstructor(),
# DiffOptMI355X.QPModel)` or `DiffOptMI355X.ConicModel`,
# src/moi_wrapper.jl:504-514) whose forward_differentiate! /
# reverse_differentiate! run the sensitivity solves on an MI355X through
# libdiffopt_mi355x.so (include/diffopt_mi355x.h).
#
# Storage, starts, input caches and every getter are those of the reference
# model they wrap (`inner`): QPModel replaces only the LHS assembly +
# `solve_system` of DiffOpt.QuadraticProgram.Model (QuadraticProgram.jl:256-282,
# 316-446, 486-496), ConicModel only `_gradient_cache`'s M and the two `lsqr`
# calls of DiffOpt.ConicProgram.Model (ConicProgram.jl:172-255, 257-394) — so
# results, sign conventions and getters are the reference's.  For the
# NonLinearProgram back-end: `mi355x_factorization` (the
# NonLinearKKTJacobianFactorization plug point) and `NLPBatch` (the batched
# sensitivity surface).  Not exercised in CI: the build image has no Julia
# (SURVEY.md §8(c)); the C-ABI it binds is exercised by the Python ctypes
# harness.  That holds for the `dual_seeds` path of QPModel too: its
# dopt_qp_reverse_duals_k call is tested through ctypes only, and for
# ConicModel's `sparse` keyword (`:split` → dopt_set_sparse(h, 2)): NOT
# EXECUTED here; tests/test_sparse_split_gpu.py runs that mode through ctypes.
module DiffOptMI355X

import DiffOpt
import LinearAlgebra
import MathOptInterface as MOI
import SparseArrays

const QP = DiffOpt.QuadraticProgram
const LIB = get(ENV, "DIFFOPT_MI355X_LIB",
                joinpath(@__DIR__, "..", "diffopt_amd", "libdiffopt_mi355x.so"))
const KIND_QP = Int32(0)
const KIND_CONIC = Int32(1)
const KIND_NLP = Int32(2)

# ---------------------------------------------------------------- handle ----
mutable struct Handle
    ptr::Ptr{Cvoid}
    n::Int
    m::Int
    p::Int
    sparse::Bool   # the handle is on the sparse route (dopt_set_sparse, or a QP above the dense cap)
end

function _check(rc::Cint, ptr::Ptr{Cvoid})
    rc == 0 && return
    rc > 0 && throw(LinearAlgebra.SingularException(Int(rc)))   # as `LHS \ RHS`
    msg = unsafe_string(ccall((:dopt_last_error, LIB), Cstring, (Ptr{Cvoid},), ptr))
    return error("diffopt_mi355x: ", msg)
end

function Handle(n::Int, m::Int, p::Int; device::Integer = 0, kind::Int32 = KIND_QP)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:dopt_create, LIB), Cint,
               (Ptr{Ptr{Cvoid}}, Cint, Int64, Int32, Int32, Int32, Int32),
               r, device, 1, n, m, p, kind)
    _check(rc, r[])
    # a QP handle with n + m + p > 8192 takes the sparse route by itself (include/diffopt_mi355x.h)
    h = Handle(r[], n, m, p, kind == KIND_QP && n + m + p > 8192)
    finalizer(h) do hh
        hh.ptr == C_NULL || ccall((:dopt_destroy, LIB), Cint, (Ptr{Cvoid},), hh.ptr)
        hh.ptr = C_NULL
    end
    return h
end

_ptr(v::Vector{Float64}) = isempty(v) ? Ptr{Float64}(C_NULL) : pointer(v)
_ptr(M::Matrix{Float64}) = isempty(M) ? Ptr{Float64}(C_NULL) : pointer(M)

# ----------------------------------------------------------------- model ----
mutable struct QPModel <: DiffOpt.AbstractModel
    inner::QP.Model                      # reference storage + getters
    model::QP.Form{Float64}              # === inner.model (DiffOpt forwards here)
    input_cache::DiffOpt.InputCache      # === inner.input_cache
    x::Vector{Float64}                   # === inner.x
    handle::Union{Nothing,Handle}
    device::Int
    staged::Any                          # (Q, G, h, A, x, λ, ν) the handle holds, or nothing
    dual_seeds::Bool                     # reverse mode reads ReverseConstraintDual (input_cache.dy)
end

# `dual_seeds = false` is the reference's behaviour: its QP back-end ignores
# ReverseConstraintDual (QuadraticProgram.jl:329 solves with [dl_dz; 0; 0]).
# With `dual_seeds = true` and a non-empty input_cache.dy, reverse_differentiate!
# solves −LHS⁻¹·[dl_dz; dl_dλ; dl_dν] (dopt_qp_reverse_duals_k); the getters are
# the reference's, unchanged.
function QPModel(; device::Integer = 0, dual_seeds::Bool = false)
    inner = QP.Model()
    return QPModel(inner, inner.model, inner.input_cache, inner.x, nothing, device, nothing, dual_seeds)
end

MOI.is_empty(m::QPModel) = MOI.is_empty(m.inner)
function MOI.empty!(m::QPModel)
    MOI.empty!(m.inner)
    m.handle = nothing
    m.staged = nothing
    return
end
MOI.get(m::QPModel, a::DiffOpt.DifferentiateTimeSec) = MOI.get(m.inner, a)
MOI.set(m::QPModel, a::MOI.ConstraintPrimalStart, ci::MOI.ConstraintIndex, v) =
    MOI.set(m.inner, a, ci, v)
MOI.set(m::QPModel, a::MOI.ConstraintDualStart, ci::MOI.ConstraintIndex, v) =
    MOI.set(m.inner, a, ci, v)               # λ = −dual(LE), ν = −dual(EQ)
MOI.get(m::QPModel, a::DiffOpt.ForwardVariablePrimal, vi::MOI.VariableIndex) =
    MOI.get(m.inner, a, vi)
MOI.get(m::QPModel, a::DiffOpt.ReverseObjectiveFunction) = MOI.get(m.inner, a)
DiffOpt._get_dA(m::QPModel, ci::MOI.ConstraintIndex) = DiffOpt._get_dA(m.inner, ci)
DiffOpt._get_db(m::QPModel, ci::MOI.ConstraintIndex) = DiffOpt._get_db(m.inner, ci)

# problem data in the MOI matrix form the reference's _gradient_cache builds
# (QuadraticProgram.jl:182-213): SparseMatrixCSC{Float64,Int64} — handed to the
# engine as is (dopt_qp_set_csc: colptr / rowval 1-based Int64, densified on
# the device), λ/ν in OptNet sign
function _problem(m::QPModel)
    inner = m.inner
    A = SparseArrays.SparseMatrixCSC{Float64,Int64}(QP._equalities(inner).coefficients)
    G = SparseArrays.SparseMatrixCSC{Float64,Int64}(QP._inequalities(inner).coefficients)
    h = Vector{Float64}(QP._inequalities(inner).constants.upper)
    n = length(inner.x)
    obj = MOI.get(inner.model,
                  MOI.ObjectiveFunction{MOI.ScalarQuadraticFunction{Float64}}())
    Q = SparseArrays.SparseMatrixCSC{Float64,Int64}(
        DiffOpt.sparse_array_representation(obj, n).quadratic_terms)
    return Q, G, h, A
end

_csc(M::SparseArrays.SparseMatrixCSC{Float64,Int64}) =
    (M.colptr, isempty(M.rowval) ? Ptr{Int64}(C_NULL) : pointer(M.rowval),
     isempty(M.nzval) ? Ptr{Float64}(C_NULL) : pointer(M.nzval), Int64(length(M.nzval)))

# Stages the model (dopt_qp_set_csc) unless the handle already holds exactly
# this data and primal-dual point: then the device factorisation from the
# previous call is reused (the reference re-factorises on every call,
# QuadraticProgram.jl:318/359; the results agree to rounding).
function _ensure!(m::QPModel)
    inner = m.inner
    n, mi, p = length(inner.x), length(inner.λ), length(inner.ν)
    h = m.handle
    if h === nothing || (h.n, h.m, h.p) != (n, mi, p)
        h = m.handle = Handle(n, mi, p; device = m.device)
        m.staged = nothing
    end
    Q, G, hv, A = _problem(m)
    key = (Q, G, hv, A, copy(inner.x), copy(inner.λ), copy(inner.ν))
    m.staged !== nothing && isequal(m.staged, key) && return h
    q, g, a = _csc(Q), _csc(G), _csc(A)
    GC.@preserve Q G hv A inner begin
        _check(ccall((:dopt_qp_set_csc, LIB), Cint,
                     (Ptr{Cvoid},
                      Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64,
                      Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64,
                      Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64,
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     h.ptr, q..., g..., a...,
                     _ptr(hv), _ptr(inner.x), _ptr(inner.λ), _ptr(inner.ν)), h.ptr)
    end
    m.staged = key
    return h
end

function _split(out::Vector{Float64}, n, mi)
    return QP.ForwardReverseCache(out[1:n], out[n+1:n+mi], out[n+mi+1:end])
end

# reverse_differentiate! (QuadraticProgram.jl:316-351)
function DiffOpt.reverse_differentiate!(m::QPModel)
    inner = m.inner
    inner.diff_time = @elapsed begin
        h = _ensure!(m)
        n, mi, p = h.n, h.m, h.p
        dl_dz = zeros(n)
        for (vi, value) in m.input_cache.dx
            dl_dz[vi.value] = value
        end
        out = Vector{Float64}(undef, n + mi + p)
        if m.dual_seeds && !isempty(m.input_cache.dy)
            # dy holds MOI duals' seeds; the engine's λ, ν are minus the MOI
            # duals (the ConstraintDualStart setters above), so the seeds flip too
            dl_dlam, dl_dnu = zeros(mi), zeros(p)
            for (ci, value) in m.input_cache.dy
                if ci isa QP.LE
                    dl_dlam[MOI.Utilities.rows(QP._inequalities(inner), ci)] = -value
                elseif ci isa QP.EQ
                    dl_dnu[MOI.Utilities.rows(QP._equalities(inner), ci)] = -value
                end
            end
            GC.@preserve dl_dz dl_dlam dl_dnu out begin
                _check(ccall((:dopt_qp_reverse_duals_k, LIB), Cint,
                             (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             h.ptr, Int32(1), dl_dz, _ptr(dl_dlam), _ptr(dl_dnu), out), h.ptr)
            end
        else
            _check(ccall((:dopt_qp_reverse, LIB), Cint,
                         (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h.ptr, dl_dz, out), h.ptr)
        end
        inner.back_grad_cache = _split(out, n, mi)
    end
    return
end

# Materialised reverse gradients of the last reverse pass (the lazy
# ReverseObjectiveFunction / ReverseConstraintFunction getters of
# QuadraticProgram.jl:448-473, :307-314 evaluated on the device for the whole
# model): (dQ, dq, dG, g_const, dA, a_const); ∂h = −g_const, ∂b = −a_const.
function reverse_gradients(m::QPModel)
    h = _ensure!(m)
    n, mi, p = h.n, h.m, h.p
    dz, dl, dn = m.inner.back_grad_cache.dz, m.inner.back_grad_cache.dλ, m.inner.back_grad_cache.dν
    rev = vcat(dz, dl, dn)
    dQ, dq = Matrix{Float64}(undef, n, n), Vector{Float64}(undef, n)
    dG, gc = Matrix{Float64}(undef, mi, n), Vector{Float64}(undef, mi)
    dA, ac = Matrix{Float64}(undef, p, n), Vector{Float64}(undef, p)
    GC.@preserve rev dQ dq dG gc dA ac begin
        _check(ccall((:dopt_qp_reverse_grads, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     h.ptr, rev, dQ, dq, _ptr(dG), _ptr(gc), _ptr(dA), _ptr(ac)), h.ptr)
    end
    return (dQ = dQ, dq = dq, dG = dG, g_const = gc, dA = dA, a_const = ac)
end

# forward_differentiate! (QuadraticProgram.jl:357-446): tangents gathered with
# the reference's own `_fill` sign rules (diff_opt.jl:594-656)
function DiffOpt.forward_differentiate!(m::QPModel)
    inner = m.inner
    inner.diff_time = @elapsed begin
        h = _ensure!(m)
        n, mi, p = h.n, h.m, h.p
        f = DiffOpt._convert(MOI.ScalarQuadraticFunction{Float64}, m.input_cache.objective)
        sa = DiffOpt.sparse_array_representation(f, n)
        dq = Vector{Float64}(sa.affine_terms)
        sets = QP._QPSets()
        db = zeros(p)
        DiffOpt._fill(isequal(MOI.EqualTo{Float64}), (::Type{MOI.EqualTo{Float64}}) -> true,
                      nothing, m.input_cache, sets, db)
        dh = zeros(mi)
        DiffOpt._fill(!isequal(MOI.EqualTo{Float64}), !isequal(MOI.GreaterThan{Float64}),
                      nothing, m.input_cache, sets, dh)
        I, J, V = Int[], Int[], Float64[]
        DiffOpt._fill(isequal(MOI.EqualTo{Float64}), isequal(MOI.GreaterThan{Float64}),
                      nothing, m.input_cache, sets, I, J, V)
        sdA = SparseArrays.sparse(I, J, V, p, n)
        I, J, V = Int[], Int[], Float64[]
        DiffOpt._fill(!isequal(MOI.EqualTo{Float64}), isequal(MOI.GreaterThan{Float64}),
                      nothing, m.input_cache, sets, I, J, V)
        sdG = SparseArrays.sparse(I, J, V, mi, n)
        out = Vector{Float64}(undef, n + mi + p)
        if h.sparse
            # sparse route: the tangents stay `sparse(I, J, V)` with their own
            # patterns, as in the reference (QuadraticProgram.jl:429-433) — no
            # dense rows × n array (dopt_qp_forward_csc).  NOT EXECUTED: the
            # project's test environment has no Julia; the Python tests exercise the entry.
            sdQ = SparseArrays.SparseMatrixCSC{Float64,Int64}(sa.quadratic_terms)
            sdG = SparseArrays.SparseMatrixCSC{Float64,Int64}(sdG)
            sdA = SparseArrays.SparseMatrixCSC{Float64,Int64}(sdA)
            GC.@preserve sdQ dq sdG dh sdA db begin
                _check(ccall((:dopt_qp_forward_csc, LIB), Cint,
                             (Ptr{Cvoid},
                              Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64},
                              Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64},
                              Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64},
                              Ptr{Float64}),
                             h.ptr, _csc(sdQ)..., _ptr(dq), _csc(sdG)..., _ptr(dh), _csc(sdA)..., _ptr(db),
                             out), h.ptr)
            end
        else
            dQ = Matrix{Float64}(sa.quadratic_terms)
            dA = Matrix{Float64}(sdA)
            dG = Matrix{Float64}(sdG)
            GC.@preserve dQ dq dG dh dA db begin
                _check(ccall((:dopt_qp_forward, LIB), Cint,
                             (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                              Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             h.ptr, _ptr(dQ), _ptr(dq), _ptr(dG), _ptr(dh), _ptr(dA), _ptr(db),
                             out), h.ptr)
            end
        end
        inner.forw_grad_cache = _split(out, n, mi)
    end
    return
end

# ------------------------------------------------ LinearAlgebraSolver ----
# The reference's narrow plug point for users who keep the stock
# QuadraticProgram.Model (QuadraticProgram.jl:475-502; exercised at
# test/moi_wrapper.jl:74-98): after `_diff`,
#   MOI.set(optimizer.diff.model, DiffOpt.QuadraticProgram.LinearAlgebraSolver(),
#           DiffOptMI355X.MI355XSolver())
# makes every `solve_system(solver, LHS, RHS, iterative)` (:335 reverse with
# LHS, :438 forward with LHS') run on the MI355X (dopt_lhs_solve): the blocked
# LU, or LSQR with IterativeSolvers' defaults when `iterative`.  A singular
# LHS raises SingularException(info) as `LHS \ RHS` does.  Per problem, like
# the plug point itself; QPModel above is the batched, assembly-on-device path.
# The reference calls solve_system twice per model (LHS, then LHS') and its
# callers loop models of one size, so the solver keeps one engine handle per
# system size rather than a dopt_create per call (ADVICE r03).  Singularity is
# the engine's rank-revealing verdict |u_ii| ≤ rows·ε·max|M|, stricter than
# `\`'s exactly-zero pivot (include/diffopt_mi355x.h, dopt_lhs_solve).
mutable struct MI355XSolver
    device::Int
    handle::Union{Nothing,Handle}
    rows::Int
    last::Any          # the matrix whose factorisation the handle holds (by identity)
    last_adj::Bool     # ... factorised as its adjoint
    last_M::Any        # ... and the contents factorised (the reuse checks them: an in-place edit refactorises)
end
MI355XSolver(; device::Integer = 0) = MI355XSolver(device, nothing, 0, nothing, false, nothing)

function _solver_handle!(s::MI355XSolver, rows::Int)
    if s.handle === nothing || s.rows != rows
        s.handle = Handle(rows, 0, 0; device = s.device, kind = KIND_NLP)
        s.rows = rows
        s.last = nothing
    end
    return s.handle
end

function QP.solve_system(s::MI355XSolver, LHS, RHS, iterative)
    rows = size(LHS, 1)
    rhs = Vector{Float64}(RHS)
    x = Vector{Float64}(undef, rows)
    h = _solver_handle!(s, rows)
    # the second call per model passes LHS' — an Adjoint wrapping the very
    # LHS just factorised (:335 then :438): answered from those factors by a
    # transposed solve (dopt_lhs_resolve), in either order — provided its
    # contents are still the ones factorised (the reference never edits LHS
    # between the two calls, but `\` has no such hazard: an edit in place
    # falls through to a fresh factorisation)
    adj = LHS isa LinearAlgebra.Adjoint || LHS isa LinearAlgebra.Transpose
    obj = adj ? parent(LHS) : LHS
    if !iterative && s.last !== nothing && obj === s.last && adj != s.last_adj &&
       (s.last_adj ? transpose(obj) == s.last_M : obj == s.last_M)
        GC.@preserve rhs x begin
            rc = ccall((:dopt_lhs_resolve, LIB), Cint,
                       (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32), h.ptr, 1, rhs, x, 1)
            s.last = nothing                 # one reuse per factorisation
            _check(rc, h.ptr)                # the factorising call's info again
        end
        return x
    end
    # LHS, or LHS' materialised (column-major); a sparse LHS is densified here
    # (the engine's dense LU: UMFPACK's sparsity is not exploited)
    M = Matrix{Float64}(LHS)
    GC.@preserve M rhs x begin
        rc = ccall((:dopt_lhs_solve, LIB), Cint,
                   (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Int32),
                   h.ptr, rows, M, 1, rhs, x, Int32(iterative))
        s.last = iterative ? nothing : obj
        s.last_adj = adj
        s.last_M = iterative ? nothing : M
        _check(rc, h.ptr)                    # rc > 0: SingularException(rc)
    end
    return x
end

# ------------------------------------------------------------ conic model ----
const CP = DiffOpt.ConicProgram

# MOI set → cone code of include/diffopt_mi355x.h (DOPT_CONE_*)
_cone_code(::Type{<:MOI.Zeros}) = Int32(0)
_cone_code(::Type{<:MOI.Nonnegatives}) = Int32(1)
_cone_code(::Type{<:MOI.Nonpositives}) = Int32(2)
_cone_code(::Type{<:MOI.SecondOrderCone}) = Int32(3)
_cone_code(::Type{<:MOI.PositiveSemidefiniteConeTriangle}) = Int32(4)
_cone_code(S::Type) = error("diffopt_mi355x: cone $S is not supported by the MI355X back-end")

mutable struct ConicModel <: DiffOpt.AbstractModel
    inner::CP.Model                      # reference storage + getters
    model::CP.Form{Float64}              # === inner.model (DiffOpt forwards here)
    input_cache::DiffOpt.InputCache      # === inner.input_cache
    x::Vector{Float64}                   # === inner.x
    s::Vector{Float64}                   # === inner.s
    y::Vector{Float64}                   # === inner.y
    handle::Union{Nothing,Handle}
    staged::Any                          # (A, b, c, x, s, y, cones) the handle holds, or nothing
    device::Int
    sparse::Union{Bool,Symbol}           # :auto (by size, density and PSD sides), false, true, or :split
end

# `sparse`: how A_moi is held on the device.  :auto — sparse (dopt_set_sparse(h, 1))
# for a large, sparse A_moi whose PSD sides are at most 64, dense otherwise; false /
# true — always dense / always mode 1 (which refuses PSD sides above 64); :split —
# dopt_set_sparse(h, DOPT_SPARSE_SPLIT): sparse A_moi under the split LSQR, PSD
# sides up to 4096 (as ConicBatch(sparse = "split") of the Python package).
function ConicModel(; device::Integer = 0, sparse::Union{Bool,Symbol} = :auto)
    sparse isa Symbol && !(sparse in (:auto, :split)) &&
        error("diffopt_mi355x: ConicModel(sparse = $sparse): expected :auto, false, true or :split")
    inner = CP.Model()
    return ConicModel(inner, inner.model, inner.input_cache, inner.x, inner.s, inner.y, nothing, nothing, device,
                      sparse)
end

const SPARSE_SPLIT = Int32(2)   # DOPT_SPARSE_SPLIT (include/diffopt_mi355x.h)

MOI.is_empty(m::ConicModel) = MOI.is_empty(m.inner)
function MOI.empty!(m::ConicModel)
    MOI.empty!(m.inner)
    m.handle = nothing
    m.staged = nothing
    return
end
MOI.supports_constraint(m::ConicModel, F::Type{MOI.VectorAffineFunction{Float64}},
                        S::Type{<:MOI.AbstractVectorSet}) = MOI.supports_constraint(m.inner, F, S)
MOI.get(m::ConicModel, a::DiffOpt.DifferentiateTimeSec) = MOI.get(m.inner, a)
MOI.set(m::ConicModel, a::MOI.ConstraintPrimalStart, ci::MOI.ConstraintIndex, v) = MOI.set(m.inner, a, ci, v)
MOI.set(m::ConicModel, a::MOI.ConstraintDualStart, ci::MOI.ConstraintIndex, v) = MOI.set(m.inner, a, ci, v)
MOI.get(m::ConicModel, a::DiffOpt.ForwardVariablePrimal, vi::MOI.VariableIndex) = MOI.get(m.inner, a, vi)
MOI.get(m::ConicModel, a::DiffOpt.ReverseObjectiveFunction) = MOI.get(m.inner, a)
MOI.get(m::ConicModel, a::MOI.ConstraintFunction, ci::MOI.ConstraintIndex) = MOI.get(m.inner, a, ci)
DiffOpt._get_dA(m::ConicModel, ci::MOI.ConstraintIndex) = DiffOpt._get_dA(m.inner, ci)
DiffOpt._get_db(m::ConicModel, ci::MOI.ConstraintIndex) = DiffOpt._get_db(m.inner, ci)

# (code, dimension) pairs in row order: the ProductOfSets layout
# (product_of_sets.jl:15-74) read back through MOI.Utilities.rows
function _cone_desc(m::ConicModel)
    cons = m.model.constraints
    desc = Tuple{Int,Int32,Int32}[]
    for (F, S) in MOI.get(m.model, MOI.ListOfConstraintTypesPresent())
        for ci in MOI.get(m.model, MOI.ListOfConstraintIndices{F,S}())
            r = MOI.Utilities.rows(cons, ci)
            push!(desc, (first(r), _cone_code(S), Int32(length(r))))
        end
    end
    sort!(desc; by = first)
    return Int32[v for (_, c, d) in desc for v in (c, d)]
end

# the engine's counterpart of `_gradient_cache` (ConicProgram.jl:172-255): A_moi
# as the MOI matrix (the diffcp sign flip is applied on the device), c negated
# for MAX_SENSE (:206-208), the NaN-start guard (:186-196) raised by the engine.
# Keyed on the full data and primal-dual point, as QPModel: any change — a new
# VariablePrimalStart (diff_opt.jl:362-370 writes m.x, which is inner.x),
# ConstraintPrimalStart / ConstraintDualStart, or a model edit — re-stages and
# re-factors; an unchanged model reuses the device factorisation.
function _ensure!(m::ConicModel)
    inner = m.inner
    Amoi = convert(SparseArrays.SparseMatrixCSC{Float64,Int64}, m.model.constraints.coefficients)
    b = Vector{Float64}(m.model.constraints.constants)
    mr, n = size(Amoi)
    if length(inner.y) < mr
        error("Some constraints are missing a value for the `ConstraintDualStart` attribute.")
    elseif length(inner.s) < mr
        error("Some constraints are missing a value for the `ConstraintPrimalStart` attribute.")
    end
    sense = MOI.get(m.model, MOI.ObjectiveSense())
    c = if sense == MOI.FEASIBILITY_SENSE
        zeros(n)
    else
        obj = MOI.get(m.model, MOI.ObjectiveFunction{MOI.ScalarAffineFunction{Float64}}())
        cc = Vector{Float64}(DiffOpt.sparse_array_representation(obj, n).terms)
        sense == MOI.MAX_SENSE ? -cc : cc
    end
    desc = _cone_desc(m)
    h = m.handle
    if h === nothing || (h.n, h.m) != (n, mr)
        h = m.handle = Handle(n, mr, 0; device = m.device, kind = KIND_CONIC)
        m.staged = nothing
        # a large, sparse A_moi stays sparse on the device (dopt_set_sparse: LSQR
        # on the matrix-free M from its CSC / CSR, as the reference's own lsqr on
        # a SparseMatrixCSC, ConicProgram.jl:323, :372) instead of an m×n dense copy
        mode = if m.sparse === :split
            SPARSE_SPLIT
        elseif m.sparse === true || (m.sparse === :auto && mr * n > 4_000_000 &&
                                     SparseArrays.nnz(Amoi) < 0.05 * mr * n && _sparse_cones_ok(desc))
            Int32(1)
        else
            Int32(0)
        end
        if mode != 0
            _check(ccall((:dopt_set_sparse, LIB), Cint, (Ptr{Cvoid}, Int32), h.ptr, mode), h.ptr)
            h.sparse = true
        end
    end
    key = (Amoi, b, c, copy(inner.x), copy(inner.s), copy(inner.y), desc)
    m.staged !== nothing && isequal(m.staged, key) && return h
    colptr, rowval, nzval, nnz = _csc(Amoi)
    GC.@preserve Amoi b c inner desc begin
        _check(ccall((:dopt_conic_set_csc, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64,
                      Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                      Ptr{Int32}, Int32),
                     h.ptr, colptr, rowval, nzval, nnz, _ptr(b), _ptr(c), _ptr(inner.x),
                     _ptr(inner.s), _ptr(inner.y), desc, Int32(length(desc) ÷ 2)), h.ptr)
        _check(ccall((:dopt_conic_factor, LIB), Cint, (Ptr{Cvoid},), h.ptr), h.ptr)
    end
    m.staged = key
    return h
end

# the one-workgroup sparse conic route (mode 1) takes PSD cones up to side 64 (include/diffopt_mi355x.h)
_sparse_cones_ok(desc) = all(k -> desc[2k-1] != 4 || desc[2k] <= 64 * 65 ÷ 2, 1:(length(desc) ÷ 2))

# forward_differentiate! (ConicProgram.jl:257-334): the tangents gathered with
# the reference's own `_fill` (dA, db in MOI layout), [du | dv | dw] from the
# device, the reference's ForwCache so ForwardVariablePrimal is its getter
function DiffOpt.forward_differentiate!(m::ConicModel)
    inner = m.inner
    inner.diff_time = @elapsed begin
        h = _ensure!(m)
        n, mr = h.n, h.m
        f = DiffOpt._convert(MOI.ScalarAffineFunction{Float64}, m.input_cache.objective)
        dc = Vector{Float64}(DiffOpt.sparse_array_representation(f, n).terms)
        db = zeros(mr)
        DiffOpt._fill(S -> false, nothing, m.input_cache, m.model.constraints.sets, db)
        I, J, V = Int[], Int[], Float64[]
        DiffOpt._fill(S -> false, nothing, m.input_cache, m.model.constraints.sets, I, J, V)
        sdA = SparseArrays.SparseMatrixCSC{Float64,Int64}(SparseArrays.sparse(I, J, V, mr, n))
        out = Vector{Float64}(undef, n + mr + 1)
        if h.sparse
            # sparse route (chosen by _ensure! because mr·n is large): dA stays
            # the reference's `sparse(dAi, dAj, dAv, lines, cols)`
            # (ConicProgram.jl:288-305) — dopt_conic_forward_csc, no dense mr × n
            # array.  NOT EXECUTED: the project's test environment has no Julia; the
            # Python tests exercise the entry.
            GC.@preserve sdA db dc begin
                _check(ccall((:dopt_conic_forward_csc, LIB), Cint,
                             (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64},
                              Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             h.ptr, _csc(sdA)..., _ptr(db), _ptr(dc), out, Ptr{Float64}(C_NULL)), h.ptr)
            end
        else
            dA = Matrix{Float64}(sdA)
            GC.@preserve dA db dc begin
                _check(ccall((:dopt_conic_forward, LIB), Cint,
                             (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                             h.ptr, _ptr(dA), _ptr(db), _ptr(dc), out, Ptr{Float64}(C_NULL)), h.ptr)
            end
        end
        inner.forw_grad_cache = CP.ForwCache(out[1:n], out[n+1:n+mr], [out[end]])
    end
    return
end

# reverse_differentiate! (ConicProgram.jl:336-394): g from the device, πz =
# [x; π(v); 1] with the reference's own projection (:375-379), so the lazy
# getters (:396-443) are the reference's
function DiffOpt.reverse_differentiate!(m::ConicModel)
    inner = m.inner
    inner.diff_time = @elapsed begin
        h = _ensure!(m)
        n, mr = h.n, h.m
        dx = zeros(n)
        for (vi, value) in m.input_cache.dx
            dx[vi.value] = value
        end
        g = Vector{Float64}(undef, n + mr + 1)
        n0 = Ptr{Float64}(C_NULL)
        _check(ccall((:dopt_conic_reverse, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     h.ptr, dx, g, n0, n0, n0), h.ptr)
        vp = DiffOpt.π(inner.y - inner.s, m.model, m.model.constraints.sets)
        inner.back_grad_cache = CP.ReverseCache(g, vcat(inner.x, vp, 1.0))
    end
    return
end

# -------------------------------------------------------- NLP factorization ----
# The NonLinearProgram back-end's own plug point: the
# `NonLinearKKTJacobianFactorization` model attribute (reference
# src/diff_opt.jl:97-112, default `_lu_with_inertia_correction` set by
# src/DiffOpt.jl:45-49) is a function `(M, model) -> K` whose result is used as
# `ldiv!(∂s, K, N)` (nlp_utilities.jl:436-442).  `mi355x_factorization`
# returns a K that lives on the MI355X: the KKT Jacobian is factorised there
# with the reference's inertia correction (M + k·1e-6·D, k ≤ 50; D = −1 on the
# constraint rows), and `ldiv!` solves all columns of N in one launch.
#
#   MOI.set(model, DiffOpt.NonLinearKKTJacobianFactorization(),
#           DiffOptMI355X.mi355x_factorization)
const NLP = DiffOpt.NonLinearProgram

struct KKTFactor
    h::Handle
    rows::Int
end

function mi355x_factorization(M::SparseArrays.SparseMatrixCSC, model::NLP.Model)
    num_w = NLP._get_num_primal_vars(model) + length(model.cache.leq_locations) +
            length(model.cache.geq_locations)                       # NonLinearProgram.jl:400-404
    num_cons = NLP._get_num_constraints(model)
    rows = size(M, 1)
    h = Handle(rows, 0, 0; kind = KIND_NLP)
    Md = Matrix{Float64}(M)                                        # column-major rows × rows
    GC.@preserve Md _check(ccall((:dopt_nlp_set_kkt, LIB), Cint,
                                 (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}),
                                 h.ptr, rows, num_w, num_cons, Md), h.ptr)
    _check(ccall((:dopt_nlp_factor, LIB), Cint, (Ptr{Cvoid},), h.ptr), h.ptr)
    corr = Ref{Int32}(0)
    _check(ccall((:dopt_nlp_get_corrections, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), h.ptr, corr), h.ptr)
    if corr[] < 0                                                  # as _inertia_correction's failure
        @warn "Inertia correction failed."
        return nothing
    end
    return KKTFactor(h, rows)
end

function LinearAlgebra.ldiv!(Y::AbstractMatrix{Float64}, K::KKTFactor, N::AbstractMatrix)
    k = size(N, 2)
    k == 0 && return Y
    Nd = Matrix{Float64}(N)                                        # rows × k = seed-major (k × 1 × rows)
    Yd = Matrix{Float64}(undef, K.rows, k)
    GC.@preserve Nd Yd _check(ccall((:dopt_nlp_kkt_solve, LIB), Cint,
                                    (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}),
                                    K.h.ptr, k, Nd, Yd), K.h.ptr)
    copyto!(Y, Yd)
    return Y
end

# ------------------------------------------------------------ NLP batches ----
# The batched NonLinearProgram surface: a batch of NLPs sharing one structure
# (the constraint kinds and which variables are bounded), each with its own
# derivatives at the solution, does the whole `_compute_sensitivity` on the
# device — the reference's `_build_sensitivity_matrices`
# (nlp_utilities.jl:181-396) → dopt_nlp_set_structure / dopt_nlp_set,
# `_lu_with_inertia_correction` (NonLinearProgram.jl:394-422) → dopt_nlp_factor,
# `forward_differentiate!` / `reverse_differentiate!` (NonLinearProgram.jl:502-582)
# → dopt_nlp_forward / dopt_nlp_reverse, ∂s (nlp_utilities.jl:457-500) →
# dopt_nlp_jacobian.  The caller evaluates the derivatives at the solution as
# the reference's MOI Nonlinear evaluator does (nlp_utilities.jl:35-92):
#   Hxx n×n×B, Hxp n×P×B (Hessian of f − sense·yᵀc), Jx c×n×B, Jp c×P×B,
#   x n×B, cval / crhs / y c×B (c(x), the set constants, MOI ConstraintDual),
#   xl / xu / yl / yu n×B (bound values and bound duals; ignored where unbounded).
# Outputs follow the Python NLPBatch (diffopt_amd/nlp.py) and the header:
#   e = NLPBatch(B, n, c, P); set_structure!(e, …); set!(e, …); factor!(e)
#   dx, ddual = nlp_forward(e, dp); dp = nlp_reverse(e; dx = seed); ∂s = nlp_jacobian(e)
mutable struct NLPBatch
    ptr::Ptr{Cvoid}
    batch::Int
    n::Int
    c::Int
    P::Int
end

function NLPBatch(batch::Integer, n::Integer, c::Integer, P::Integer; device::Integer = 0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:dopt_create, LIB), Cint,
               (Ptr{Ptr{Cvoid}}, Cint, Int64, Int32, Int32, Int32, Int32),
               r, device, batch, n, c, P, KIND_NLP)
    _check(rc, r[])
    e = NLPBatch(r[], Int(batch), Int(n), Int(c), Int(P))
    finalizer(e) do ee
        ee.ptr == C_NULL || ccall((:dopt_destroy, LIB), Cint, (Ptr{Cvoid},), ee.ptr)
        ee.ptr = C_NULL
    end
    return e
end

"""
    set_structure!(e, con_kind, has_low, has_up, sense)

`con_kind[i]`: 0 `EqualTo`, 1 `GreaterThan`, 2 `LessThan` for NLP row i (the
reference's constraint order); `has_low` / `has_up`: which variables carry a
`VariableIndex`-in-`GreaterThan` / `LessThan` bound; `sense` = +1 (MIN) / −1 (MAX).
"""
function set_structure!(e::NLPBatch, con_kind::AbstractVector{<:Integer}, has_low::AbstractVector{Bool},
                        has_up::AbstractVector{Bool}, sense::Integer)
    ck = Int32.(con_kind)
    lo = Int8.(has_low)
    up = Int8.(has_up)
    GC.@preserve ck lo up _check(ccall((:dopt_nlp_set_structure, LIB), Cint,
                                       (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int8}, Ptr{Int8}, Int32),
                                       e.ptr, ck, lo, up, sense), e.ptr)
    return e
end

_fptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
_dense(a) = a === nothing ? nothing : convert(Array{Float64}, a)

function set!(e::NLPBatch, Hxx, Hxp, Jx, Jp, x, cval, crhs, y;
              xl = nothing, xu = nothing, yl = nothing, yu = nothing)
    A = map(_dense, (Hxx, Hxp, Jx, Jp, x, cval, crhs, y, xl, xu, yl, yu))
    GC.@preserve A _check(ccall((:dopt_nlp_set, LIB), Cint, (Ptr{Cvoid}, ntuple(_ -> Ptr{Float64}, 12)...),
                                e.ptr, map(_fptr, A)...), e.ptr)
    return e
end

"Factorise every problem's KKT system; returns the inertia corrections (0 none, k > 0, −1 failed)."
function factor!(e::NLPBatch)
    _check(ccall((:dopt_nlp_factor, LIB), Cint, (Ptr{Cvoid},), e.ptr), e.ptr)
    corr = Vector{Int32}(undef, e.batch)
    _check(ccall((:dopt_nlp_get_corrections, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), e.ptr, corr), e.ptr)
    return corr
end

"(rows, num_w, c, nlo, nup, nlow_primal, nup_primal) of the KKT system."
function nlp_layout(e::NLPBatch)
    l = Vector{Int32}(undef, 7)
    _check(ccall((:dopt_nlp_get_layout, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), e.ptr, l), e.ptr)
    return Tuple(Int.(l))
end

_ndual(e::NLPBatch) = (l = nlp_layout(e); l[3] + l[6] + l[7])

"Forward mode (NonLinearProgram.jl:502-528): dp P×B → (dx n×B, ddual (c+nlow+nup)×B)."
function nlp_forward(e::NLPBatch, dp::AbstractMatrix)
    dpd = convert(Matrix{Float64}, dp)
    dx = Matrix{Float64}(undef, e.n, e.batch)
    dd = Matrix{Float64}(undef, _ndual(e), e.batch)
    GC.@preserve dpd dx dd _check(ccall((:dopt_nlp_forward, LIB), Cint,
                                        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                        e.ptr, dpd, dx, dd), e.ptr)
    return dx, dd
end

"Reverse mode (NonLinearProgram.jl:530-582): seeds dx n×B and/or ddual → dp P×B."
function nlp_reverse(e::NLPBatch; dx = nothing, ddual = nothing)
    a, d = _dense(dx), _dense(ddual)
    dp = Matrix{Float64}(undef, e.P, e.batch)
    GC.@preserve a d dp _check(ccall((:dopt_nlp_reverse, LIB), Cint,
                                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                     e.ptr, _fptr(a), _fptr(d), dp), e.ptr)
    return dp
end

"Both modes against the same factors in one call (one pass over them): dp, seeds → (dx, ddual, dp_out)."
function nlp_forward_reverse(e::NLPBatch, dp::AbstractMatrix; dx = nothing, ddual = nothing)
    dpd = convert(Matrix{Float64}, dp)
    a, d = _dense(dx), _dense(ddual)
    ox = Matrix{Float64}(undef, e.n, e.batch)
    od = Matrix{Float64}(undef, _ndual(e), e.batch)
    op = Matrix{Float64}(undef, e.P, e.batch)
    GC.@preserve dpd a d ox od op _check(ccall((:dopt_nlp_forward_reverse, LIB), Cint,
                                               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                                                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                               e.ptr, dpd, _fptr(a), _fptr(d), ox, od, op), e.ptr)
    return ox, od, op
end

"∂s per problem (nlp_utilities.jl:457-500): rows × P × B."
function nlp_jacobian(e::NLPBatch)
    rows = nlp_layout(e)[1]
    ds = Array{Float64}(undef, rows, e.P, e.batch)
    GC.@preserve ds _check(ccall((:dopt_nlp_jacobian, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), e.ptr, ds), e.ptr)
    return ds
end

end # module

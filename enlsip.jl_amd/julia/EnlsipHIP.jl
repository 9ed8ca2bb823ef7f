# EnlsipHIP.jl — thin ccall glue that plugs libenlsip_gn.so underneath Enlsip.jl's
# Gauss-Newton subproblem (gn_search_direction + the QR lines of update_working_set), leaving
# CnlsModel / solve! and everything above the seam unchanged.
#
# STATUS: written against include/enlsip_gn.h and the reference sources, but NOT executed:
# no Julia toolchain exists in the build container or on the GPU box (SURVEY.md §0, §8c).  The
# same C ABI is exercised end to end by the ctypes host mirror (enlsip.jl_amd/python) and
# tests/test_gpu_parity.py; INTEGRATION.md shows how a maintainer wires this file in.
#
# Seam (reference lines):
#   update_working_set   src/enlsip_functions.jl:686-795   (QR lines :700, 722-725, 740-743, 758-762, 768-771, 786-789)
#   gn_search_direction  src/enlsip_functions.jl:206-234
#   sub_search_direction src/enlsip_functions.jl:116-153   (re-entered at :1253)
module EnlsipHIP

using LinearAlgebra

const LIB = get(ENV, "ENLSIP_GN_LIB", joinpath(@__DIR__, "..", "lib", "libenlsip_gn.so"))

const FACTOR_A = Cint(0)
const FACTOR_L11 = Cint(1)
const FACTOR_J2 = Cint(2)

struct Opts
    device::Int32
    flags::Int32
    panel_width::Int32
    tile_rows::Int32
    stream::Ptr{Cvoid}
end

struct Info
    rankA::Int64
    rankJ2::Int64
    code::Int64
    dimA::Int64
    dimJ2::Int64
    status::Int64
end

mutable struct Handle
    ptr::Ptr{Cvoid}
    function Handle(; device::Integer=-1, flags::Integer=0)
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        opts = Ref(Opts(Int32(device), Int32(flags), Int32(0), Int32(0), C_NULL))
        rc = ccall((:enlsip_gn_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{Opts}), ref, opts)
        rc == 0 || error("enlsip_gn_create failed with code $rc: " *
                         unsafe_string(ccall((:enlsip_gn_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
        h = new(ref[])
        finalizer(x -> ccall((:enlsip_gn_destroy, LIB), Cint, (Ptr{Cvoid},), x.ptr), h)
        return h
    end
end

function check(h::Handle, rc::Integer)
    rc == 0 && return
    msg = unsafe_string(ccall((:enlsip_gn_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr))
    error("libenlsip_gn error $rc: $msg")
end

# QRPivoted-like shim backed by the device-resident factors of the last solve on `h`
# (valid until the next solve).  Supports exactly what the reference's consumers use:
# F.R, F.p, F.P, F.Q' * v, F.Q * v  (src/enlsip_functions.jl:461-537, 1118-1291).
struct DeviceQR
    h::Handle
    which::Cint
    rows::Int      # length of vectors Q acts on
end

function factor_shape(F::DeviceQR)
    r = Ref{Int64}(0); c = Ref{Int64}(0)
    check(F.h, ccall((:enlsip_gn_factor_shape, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{Int64}, Ref{Int64}),
                     F.h.ptr, F.which, 0, r, c))
    return r[], c[]
end

function Base.getproperty(F::DeviceQR, s::Symbol)
    if s === :R
        r, c = factor_shape(F)
        R = zeros(Float64, max(r, 1), c)
        GC.@preserve R check(F.h, ccall((:enlsip_gn_get_R, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Int64),
                                        getfield(F, :h).ptr, getfield(F, :which), 0, R, max(r, 1)))
        return R[1:r, :]
    elseif s === :p
        _, c = factor_shape(F)
        p = zeros(Int64, c)
        c > 0 && GC.@preserve p check(getfield(F, :h), ccall((:enlsip_gn_get_jpvt, LIB), Cint,
                                      (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}), getfield(F, :h).ptr, getfield(F, :which), 0, p))
        return p
    elseif s === :P
        p = F.p
        n = length(p)
        P = zeros(Float64, n, n)
        for i in 1:n
            P[p[i], i] = 1.0
        end
        return P
    elseif s === :Q
        return DeviceQ(F, false)
    else
        return getfield(F, s)
    end
end

struct DeviceQ
    F::DeviceQR
    adj::Bool
end
Base.adjoint(Q::DeviceQ) = DeviceQ(Q.F, !Q.adj)

function Base.:*(Q::DeviceQ, v::AbstractVector{Float64})
    out = Vector{Float64}(v)
    h = getfield(Q.F, :h)
    GC.@preserve out begin
        rc = Q.adj ?
            ccall((:enlsip_gn_apply_qt, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}), h.ptr, getfield(Q.F, :which), 0, out) :
            ccall((:enlsip_gn_apply_q, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}), h.ptr, getfield(Q.F, :which), 0, out)
        check(h, rc)
    end
    return out
end

# M * F.Q and M * F.Q' — what the reference's consumers write as `J * F_A.Q` (src/enlsip_functions.jl:384, :526, :1249), so that
# those lines run UNMODIFIED on a DeviceQR.  `F_A.Q` applied from the right to a matrix with as many rows as the J of the last
# solve is one launch of the library's J*Q1 kernel on the resident reflectors (enlsip_gn_matrix_times_QA: M is staged, nothing
# about it needs to be resident); every other combination (F_L11 / F_J2, adjoints, other row counts) falls back to one
# `Q' * row` per row of M — correct for any M, slow for tall ones, and not on any path the reference takes.
function Base.:*(M::AbstractMatrix{Float64}, Q::DeviceQ)
    F = Q.F
    h = getfield(F, :h)
    rows, cols = size(M)
    cols == getfield(F, :rows) || throw(DimensionMismatch("matrix has $cols columns, Q acts on vectors of length $(getfield(F, :rows))"))
    if getfield(F, :which) == FACTOR_A && !Q.adj
        Md = Matrix{Float64}(M)
        out = zeros(Float64, rows, cols)
        rc = GC.@preserve Md out ccall((:enlsip_gn_matrix_times_QA, LIB), Cint,
                                       (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                                       h.ptr, 0, rows, Md, max(rows, 1), out, max(rows, 1))
        rc == 0 && return out
        rc == -3 || check(h, rc)         # -3: rows differ from the resident plan's m — generic path below
    end
    # (M Q)' = Q' M'  and  (M Q')' = Q M': one vector application per row of M
    out = Matrix{Float64}(undef, rows, cols)
    Qt = DeviceQ(F, !Q.adj)
    for i in 1:rows
        out[i, :] = Qt * Vector{Float64}(M[i, :])
    end
    return out
end

# J * F_A.Q  (src/enlsip_functions.jl:219, :526, :1249): served from the device instead of a second dormqr
function jq1(h::Handle, m::Integer, n::Integer)
    out = zeros(Float64, m, n)
    GC.@preserve out check(h, ccall((:enlsip_gn_get_JQ1, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), h.ptr, 0, out, m))
    return out
end

"""
    gn_search_direction_hip!(h, J, rx, A_active, cx, ε_rank, current_iter) -> p_gn, F_A, F_L11, F_J2

Replaces, in `update_working_set`, every occurrence of

    F_A = qr(C.A', ColumnNorm()); rankA = pseudo_rank(diag(F_A.R), ε_rank)
    F_L11 = qr(F_A.R', ColumnNorm())
    p_gn[:], F_J2 = gn_search_direction(J, rx, C.cx, F_A, F_L11, rankA, W.t, ε_rank, iter_k)

(src/enlsip_functions.jl:722-725, 740-743, 758-762, 768-771, 786-789) by one call into the HIP
library, and writes the same `Iteration` fields gn_search_direction writes (:226-231).
`A_active` is `C.A` (t x n); its transpose is materialised because the ABI wants `C.A'` column-major.
"""
function gn_search_direction_hip!(h::Handle, J::Matrix{Float64}, rx::Vector{Float64}, A_active::Matrix{Float64},
                                  cx::Vector{Float64}, ε_rank::Float64, current_iter)
    m, n = size(J)
    t = size(A_active, 1)
    At = Matrix{Float64}(transpose(A_active))          # n x t, column-major
    p = zeros(Float64, n); b = zeros(Float64, t); d = zeros(Float64, m)
    info = Ref(Info(0, 0, 0, 0, 0, 0))
    jA = zeros(Int64, t); jL = zeros(Int64, min(n, t)); jJ = zeros(Int64, n)
    GC.@preserve J rx At cx p b d jA jL jJ begin
        rc = ccall((:enlsip_gn_solve, LIB), Cint,
                   (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
                    Ptr{Float64}, Float64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Info},
                    Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                   h.ptr, m, n, t, J, m, rx, At, max(n, 1), cx, ε_rank, -1, -1, p, b, d, info, jA, jL, jJ)
        check(h, rc)
    end
    i = info[]
    (i.status & 1) != 0 && throw(LinearAlgebra.SingularException(0))   # Julia's `\` would have thrown
    current_iter.rankA = i.rankA
    current_iter.rankJ2 = i.rankJ2
    current_iter.dimA = i.rankA
    current_iter.dimJ2 = i.rankJ2
    current_iter.b_gn = b
    current_iter.d_gn = d
    return p, DeviceQR(h, FACTOR_A, n), DeviceQR(h, FACTOR_L11, t), DeviceQR(h, FACTOR_J2, m)
end

"""
    d_gn_prefix(d_gn, k, n, rankA) -> view(d_gn, 1:k)

The leading `n - rankA` entries of `d_gn` agree with the reference's up to a sign per entry (the thin Q of `F_J2` is unique up
to column signs once the pivots are fixed), so every norm of a prefix `d_gn[1:k]` with `k <= n - rankA` is the reference's; the
entries beyond are an orthogonal transform of the reference's tail and only their norm as a whole is the same (SURVEY §7 H1).
The reference slices such prefixes in `search_direction_analys` (`d_gn[1:prev_dimJ2m1]`, src/enlsip_functions.jl:1230-1231),
`choose_subspace_dimensions` (:1166-1169) and `check_termination_criteria` (:2448-2452); with `dimJ2 <= n - t_prev` they never
reach past `n - rankA`.  Route those slices through this helper when the HIP backend is active: it asserts the bound instead
of silently mixing tail components into a norm.
"""
function d_gn_prefix(d_gn::AbstractVector{Float64}, k::Integer, n::Integer, rankA::Integer)
    @assert 0 <= k <= n - rankA "d_gn[1:$k] reaches past n - rankA = $(n - rankA): only the norm of the whole tail is defined there (src/enlsip_functions.jl:1230-1231)"
    return view(d_gn, 1:k)
end

"""
    sub_search_direction_hip(h, m, n, t, dimA, dimJ2, code) -> p, b, d

Re-entry of `sub_search_direction` on the resident factors with truncated dimensions
(src/enlsip_functions.jl:1253, subspace minimisation).  SURVEY §7 H1: callers that slice
`d_gn[1:k]` must keep `k <= n - rankA`: `d_gn_prefix` above asserts it.
"""
function sub_search_direction_hip(h::Handle, m::Integer, n::Integer, t::Integer, dimA::Integer, dimJ2::Integer, code::Integer)
    p = zeros(Float64, n); b = zeros(Float64, t); d = zeros(Float64, m)
    GC.@preserve p b d check(h, ccall((:enlsip_gn_resolve, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h.ptr, 0, dimA, dimJ2, code, p, b, d))
    return p, b, d
end

"""
    first_lagrange_mult_estimate_hip!(h, λ, ∇fx, scaling_done, diag_scale, iter, ε_rank)

Device form of `first_lagrange_mult_estimate!` (src/enlsip_functions.jl:461-508) on the resident `F_A` and `cx`
of the last solve on `h`; writes `λ` and `iter.grad_res`.  Pass `∇fx = nothing` to use `Jᵀ rx` of the resident
`J`, `rx` (then `gradient_hip(h, n)` returns the same vector for the caller).
"""
function first_lagrange_mult_estimate_hip!(h::Handle, λ::Vector{Float64}, ∇fx::Union{Nothing,Vector{Float64}},
                                           scaling_done::Bool, diag_scale::Vector{Float64}, iter, ε_rank::Float64)
    gres = Ref{Float64}(0.0)
    g = ∇fx === nothing ? Ptr{Float64}(C_NULL) : pointer(∇fx)
    ds = scaling_done ? pointer(diag_scale) : Ptr{Float64}(C_NULL)
    GC.@preserve λ ∇fx diag_scale check(h, ccall((:enlsip_gn_first_lagrange, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{Float64}),
        h.ptr, 0, g, ds, ε_rank, λ, gres))
    iter.grad_res = gres[]
    return
end

"""
    second_lagrange_mult_estimate_hip!(h, λ, p_gn, scaling, diag_scale, ε_rank=sqrt(eps()))

Device form of `second_lagrange_mult_estimate!` (:514-537): uses the resident `J1 = (J*F_A.Q)[:, 1:t]` instead of
recomputing `J*F_A.Q` (:526).
"""
function second_lagrange_mult_estimate_hip!(h::Handle, λ::Vector{Float64}, p_gn::Vector{Float64}, scaling::Bool,
                                            diag_scale::Vector{Float64}, ε_rank::Float64=sqrt(eps(Float64)))
    ds = scaling ? pointer(diag_scale) : Ptr{Float64}(C_NULL)
    GC.@preserve λ p_gn diag_scale check(h, ccall((:enlsip_gn_second_lagrange, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}),
        h.ptr, 0, p_gn, ds, ε_rank, λ))
    return
end

"""    gradient_hip(h, n) -> Jᵀ rx of the J, rx of the last solve (src/enlsip_functions.jl:2690)"""
function gradient_hip(h::Handle, n::Integer)
    g = zeros(Float64, n)
    GC.@preserve g check(h, ccall((:enlsip_gn_gradient, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}), h.ptr, 0, g))
    return g
end

"""    factor_constraints_hip!(h, m, A, cx, ε_rank) -> (rankA, F_A, F_L11)

The constraint stage alone (src/enlsip_functions.jl:700, :768-769): leaves `F_A`, `F_L11` resident for
`first_lagrange_mult_estimate_hip!` (:704) before any subproblem solve.  `m` = rows of the solve that follows.
"""
function factor_constraints_hip!(h::Handle, m::Integer, A::Matrix{Float64}, cx::Vector{Float64}, ε_rank::Float64)
    t, n = size(A)
    At = Matrix(transpose(A))
    info = Ref(Info(0, 0, 0, 0, 0, 0))
    GC.@preserve At cx check(h, ccall((:enlsip_gn_factor_constraints, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ref{Info}),
        h.ptr, m, n, t, At, max(n, 1), cx, ε_rank, info))
    return info[].rankA, DeviceQR(h, FACTOR_A, n), DeviceQR(h, FACTOR_L11, t)
end

"""    gn_search_direction_factored_hip!(h, J, rx, t, ε_rank, iter_k) -> (p_gn, F_A, F_L11, F_J2)

The solve of `update_working_set`'s `s == 0` branch (:768-771) right after `factor_constraints_hip!` with the same working set:
the resident `F_A`, `F_L11`, `b`, `p1` are reused, only `J` and `rx` are sent.
"""
function gn_search_direction_factored_hip!(h::Handle, J::Matrix{Float64}, rx::Vector{Float64}, t::Integer, ε_rank::Float64, iter_k)
    m, n = size(J)
    kA = min(n, t)
    p = zeros(Float64, n); b = zeros(Float64, max(t, 1)); d = zeros(Float64, m)
    jA = zeros(Int64, max(t, 1)); jL = zeros(Int64, max(kA, 1)); jJ = zeros(Int64, n)
    info = Ref(Info(0, 0, 0, 0, 0, 0))
    GC.@preserve J rx p b d jA jL jJ check(h, ccall((:enlsip_gn_solve_factored, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Int64, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ref{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, m, n, t, J, m, rx, ε_rank, -1, p, b, d, info, jA, jL, jJ))
    iter_k.rankA = info[].rankA; iter_k.rankJ2 = info[].rankJ2
    iter_k.dimA = info[].dimA; iter_k.dimJ2 = info[].dimJ2
    iter_k.b_gn = b[1:t]; iter_k.d_gn = d
    return p, DeviceQR(h, FACTOR_A, n), DeviceQR(h, FACTOR_L11, t), DeviceQR(h, FACTOR_J2, m)
end

"""    jacobian_times_hip(h, p, m, t) -> (J*p, C.A*p) on the J and A of the last solve (src/enlsip_functions.jl:2226-2229)"""
function jacobian_times_hip(h::Handle, p::Vector{Float64}, m::Integer, t::Integer)
    Jp = zeros(Float64, m); Ap = zeros(Float64, t)
    GC.@preserve p Jp Ap check(h, ccall((:enlsip_gn_jacobian_times, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, 0, p, Jp, t > 0 ? pointer(Ap) : Ptr{Float64}(C_NULL)))
    return Jp, Ap
end

"""    full_constraints_times_hip(h, A, p) -> A * p

The product of the line-search set-up with the FULL constraint Jacobian, inactive rows included (`Ap = A * p`,
src/enlsip_functions.jl:2227), on the device: `A` (l x n) is staged, nothing about it has to be resident.
"""
function full_constraints_times_hip(h::Handle, A::Matrix{Float64}, p::Vector{Float64})
    l, n = size(A)
    Ap = zeros(Float64, l)
    l == 0 && return Ap
    GC.@preserve A p Ap check(h, ccall((:enlsip_gn_full_constraints_times, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}), h.ptr, l, n, A, l, p, Ap))
    return Ap
end

"""    route(h) -> Vector{String}: the kernel-selection branches the last solve on `h` took (enlsip_gn_get_route; diagnostics)"""
function route(h::Handle)
    mask = Ref{UInt64}(0)
    check(h, ccall((:enlsip_gn_get_route, LIB), Cint, (Ptr{Cvoid}, Ref{UInt64}), h.ptr, mask))
    names = String[]
    bit = 0
    while true
        nm = ccall((:enlsip_gn_route_name, LIB), Ptr{UInt8}, (Cint,), bit)
        nm == C_NULL && break
        (mask[] >> bit) & 1 == 1 && push!(names, unsafe_string(nm))
        bit += 1
    end
    return names
end

"""    tsqr_exchange(h) -> (transport, ranks, rank_tags_seen) of the last `gn_search_direction_tsqr_hip` on `h`:
`rank_tags_seen == ranks` on every rank means one correctly tagged message from each rank arrived (transport 1 = RCCL)."""
function tsqr_exchange(h::Handle)
    tr = Ref{Cint}(-1); rk = Ref{Cint}(0); seen = Ref{Cint}(-1)
    check(h, ccall((:enlsip_gn_tsqr_get_exchange, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), h.ptr, tr, rk, seen))
    return Int(tr[]), Int(rk[]), Int(seen[])
end

"""    diagR(F::DeviceQR) -> diag(F.R) without moving the triangle (what `pseudo_rank(diag(F.R), ε)` needs, :768, :224)"""
function diagR(F::DeviceQR)
    r, c = factor_shape(F)
    k = min(r, c)
    dg = zeros(Float64, max(k, 1))
    GC.@preserve dg check(getfield(F, :h), ccall((:enlsip_gn_get_diagR, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}),
                                                 getfield(F, :h).ptr, getfield(F, :which), 0, dg))
    return dg[1:k]
end

"""    gn_search_direction_batched_hip(h, Js, rxs, As, cxs, ε_rank) -> (P, infos)

New capability (no reference counterpart): `B` independent subproblems of one shape in one call — `Js` is `m×n×B`, `rxs` `m×B`,
`As` `t×n×B` (the active constraint Jacobians), `cxs` `t×B`.  Returns the directions as the columns of `P` (`n×B`) and the
per-problem `Info` records.  Factors stay resident; pass `prob` to the accessors of the C ABI to reach problem `k`.
"""
function gn_search_direction_batched_hip(h::Handle, Js::Array{Float64,3}, rxs::Matrix{Float64}, As::Array{Float64,3},
                                         cxs::Matrix{Float64}, ε_rank::Float64)
    m, n, B = size(Js)
    t = size(As, 1)
    kA = min(n, t)
    Ats = permutedims(As, (2, 1, 3))                     # n×t×B: every slice is C.A' column-major
    P = zeros(Float64, n, B); b = zeros(Float64, max(t, 1), B); d = zeros(Float64, m, B)
    jA = zeros(Int64, max(t, 1), B); jL = zeros(Int64, max(kA, 1), B); jJ = zeros(Int64, n, B)
    infos = fill(Info(0, 0, 0, 0, 0, 0), B)
    GC.@preserve Js rxs Ats cxs P b d jA jL jJ infos check(h, ccall((:enlsip_gn_solve_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, m, n, t, Js, m, m * n, rxs, Ats, max(n, 1), n * t, cxs, ε_rank, P, b, d, infos, jA, jL, jJ))
    return P, infos
end

"""    gn_search_direction_batched_hip(h, Js, rxs, As::Vector{Matrix{Float64}}, cxs, ε_rank) -> (P, infos)

The ragged form: every problem brings its own active Jacobian `As[k]` (`t_k×n`, different row counts after
update_working_set, src/enlsip_functions.jl:686-795) and `cxs[k]` (`t_k`).  They are packed into `t_max` padding and solved in
one call of enlsip_gn_solve_batched_ragged; problem `k`'s results are those of its own `t_k`.
"""
function gn_search_direction_batched_hip(h::Handle, Js::Array{Float64,3}, rxs::Matrix{Float64}, As::Vector{Matrix{Float64}},
                                         cxs::Vector{Vector{Float64}}, ε_rank::Float64)
    m, n, B = size(Js)
    t = Int64[size(A, 1) for A in As]
    t_max = B > 0 ? maximum(t) : 0
    kA = min(n, t_max)
    Ats = zeros(Float64, n, max(t_max, 1), B)            # n×t_max×B: slice k holds C.A' of problem k in its first t_k columns
    cxp = zeros(Float64, max(t_max, 1), B)
    for k in 1:B
        t[k] > 0 || continue
        Ats[:, 1:t[k], k] = permutedims(As[k], (2, 1))
        cxp[1:t[k], k] = cxs[k]
    end
    P = zeros(Float64, n, B); b = zeros(Float64, max(t_max, 1), B); d = zeros(Float64, m, B)
    jA = zeros(Int64, max(t_max, 1), B); jL = zeros(Int64, max(kA, 1), B); jJ = zeros(Int64, n, B)
    infos = fill(Info(0, 0, 0, 0, 0, 0), B)
    GC.@preserve Js rxs t Ats cxp P b d jA jL jJ infos check(h, ccall((:enlsip_gn_solve_batched_ragged, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
         Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, m, n, t_max, t, Js, m, m * n, rxs, Ats, max(n, 1), n * max(t_max, 1), cxp, ε_rank, P, b, d, infos, jA, jL, jJ))
    return P, infos
end

# ---- the batched constraint stage and the solve that goes on with it (src/enlsip_functions.jl:700-704, then :725 / :771) ----------

# n×t_max×B / t_max×B padded copies of every problem's C.A' and cx (slice k: its first t_k columns / entries)
function pack_working_sets(n::Integer, t_max::Integer, As::Vector{Matrix{Float64}}, cxs::Vector{Vector{Float64}})
    B = length(As)
    t = Int64[size(A, 1) for A in As]
    all(tk -> tk <= t_max, t) || error("a working set has more than t_max = $t_max constraints")
    Ats = zeros(Float64, n, max(t_max, 1), B)
    cxp = zeros(Float64, max(t_max, 1), B)
    for k in 1:B
        t[k] > 0 || continue
        Ats[:, 1:t[k], k] = permutedims(As[k], (2, 1))
        cxp[1:t[k], k] = cxs[k]
    end
    return t, Ats, cxp
end

"""    factor_constraints_batched_hip(h, m, n, t_max, As, cxs, ε_rank) -> infos

`F_A = qr(C.A', ColumnNorm())` (src/enlsip_functions.jl:700), rankA and `F_L11` (:768-769) of every problem of a batch, nothing about
J: what a batched update_working_set needs before the deletion test (:704, `first_lagrange_batched_hip` with `grad_fx`).  `t_max` is
the padding both calls of the pair share; `m` the row count of the solve that follows."""
function factor_constraints_batched_hip(h::Handle, m::Integer, n::Integer, t_max::Integer, As::Vector{Matrix{Float64}},
                                        cxs::Vector{Vector{Float64}}, ε_rank::Float64)
    B = length(As)
    t, Ats, cxp = pack_working_sets(n, t_max, As, cxs)
    infos = fill(Info(0, 0, 0, 0, 0, 0), B)
    GC.@preserve t Ats cxp infos check(h, ccall((:enlsip_gn_factor_constraints_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64, Ptr{Info}),
        h.ptr, B, m, n, t_max, t, Ats, max(n, 1), n * max(t_max, 1), cxp, ε_rank, infos))
    return infos
end

"""    gn_search_direction_factored_batched_hip(h, Js, rxs, t_max, As, cxs, refactor, ε_rank) -> (P, infos)

The Jacobian side right after `factor_constraints_batched_hip` (same `t_max`): problems with `refactor[k]` false keep their
constraint stage (`As[k]` must have the row count it was factored with and is not read), the others get theirs again from `As[k]`,
`cxs[k]` first.  Results per problem as `gn_search_direction_batched_hip` on the final working sets."""
function gn_search_direction_factored_batched_hip(h::Handle, Js::Array{Float64,3}, rxs::Matrix{Float64}, t_max::Integer,
                                                  As::Vector{Matrix{Float64}}, cxs::Vector{Vector{Float64}},
                                                  refactor::AbstractVector{Bool}, ε_rank::Float64)
    m, n, B = size(Js)
    kA = min(n, t_max)
    t, Ats, cxp = pack_working_sets(n, t_max, As, cxs)
    flags = Int64[r ? 1 : 0 for r in refactor]
    P = zeros(Float64, n, B); b = zeros(Float64, max(t_max, 1), B); d = zeros(Float64, m, B)
    jA = zeros(Int64, max(t_max, 1), B); jL = zeros(Int64, max(kA, 1), B); jJ = zeros(Int64, n, B)
    infos = fill(Info(0, 0, 0, 0, 0, 0), B)
    GC.@preserve Js rxs t flags Ats cxp P b d jA jL jJ infos check(h, ccall((:enlsip_gn_solve_factored_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64,
         Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, m, n, t_max, t, flags, Js, m, m * n, rxs, Ats, max(n, 1), n * max(t_max, 1), cxp, ε_rank, P, b, d, infos, jA, jL, jJ))
    return P, infos
end

"""    gn_search_direction_changed_batched_hip!(h, P, infos, m, t_max, As, cxs, changed, ε_rank) -> (P, infos)

Only the problems whose working set changed, in place, on the fully solved ragged batch that is resident (the undo of
src/enlsip_functions.jl:728-743, a second-order deletion :745-762 / :773-790): constraint stage and Jacobian side again for the
problems with `changed[k]`, from the resident `J`, `rx` and `As[k]`, `cxs[k]`; the others (`As[k]` must have the row count they are
resident with) are not touched, and their columns of `P` and entries of `infos` stay as they are."""
function gn_search_direction_changed_batched_hip!(h::Handle, P::Matrix{Float64}, infos::Vector{Info}, m::Integer, t_max::Integer,
                                                  As::Vector{Matrix{Float64}}, cxs::Vector{Vector{Float64}},
                                                  changed::AbstractVector{Bool}, ε_rank::Float64)
    n, B = size(P)
    kA = min(n, t_max)
    t, Ats, cxp = pack_working_sets(n, t_max, As, cxs)
    flags = Int64[c ? 1 : 0 for c in changed]
    b = zeros(Float64, max(t_max, 1), B); d = zeros(Float64, m, B)
    jA = zeros(Int64, max(t_max, 1), B); jL = zeros(Int64, max(kA, 1), B); jJ = zeros(Int64, n, B)
    GC.@preserve t flags Ats cxp P b d jA jL jJ infos check(h, ccall((:enlsip_gn_solve_changed_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, m, n, t_max, t, flags, Ats, max(n, 1), n * max(t_max, 1), cxp, ε_rank, P, b, d, infos, jA, jL, jJ))
    return P, infos
end

"""    gn_search_direction_changed_batched_dev_hip(h, B, m, n, t_max, t, changed, dAt, ldat, strideAt, dcx, ε_rank, dp, db, dd, dinfo)

The same with DEVICE buffers: `dAt`, `ldat`, `strideAt`, `dcx` are those of the resident solve, the changed slots rewritten in place;
`t` and `changed` stay host arrays; only the changed problems' output slots are written."""
function gn_search_direction_changed_batched_dev_hip(h::Handle, B::Integer, m::Integer, n::Integer, t_max::Integer, t::Vector{Int64},
                                                     changed::AbstractVector{Bool}, dAt::Ptr{Float64}, ldat::Integer,
                                                     strideAt::Integer, dcx::Ptr{Float64}, ε_rank::Float64, dp::Ptr{Float64},
                                                     db::Ptr{Float64}, dd::Ptr{Float64}, dinfo::Ptr{Info})
    flags = Int64[c ? 1 : 0 for c in changed]
    GC.@preserve t flags check(h, ccall((:enlsip_gn_solve_changed_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, m, n, t_max, t, flags, dAt, ldat, strideAt, dcx, ε_rank, dp, db, dd, dinfo, Ptr{Int64}(0), Ptr{Int64}(0), Ptr{Int64}(0)))
    return nothing
end

"""    jacobian_resolved_hip(h) -> problems the Jacobian-side kernels of the last solve on `h` were launched over"""
function jacobian_resolved_hip(h::Handle)
    c = Ref{Int64}(0)
    check(h, ccall((:enlsip_gn_get_jacobian_resolved, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h.ptr, c))
    return Int(c[])
end

# ---- the consumers of a batched solve over a range of its problems (one call, a fixed number of launches) ----------------------
#
# A batched outer iteration: solve (ragged), first estimate over the batch, the host deletion test of update_working_set
# (src/enlsip_functions.jl:700-704), then a ragged re-solve of the problems whose working set changed.  Problem `prob0 + j`
# (0-based, as the C ABI counts) is column `j + 1` of every array; lambda and Ap have `t_max` rows, zero past a problem's own t.
# status: 0, 1 singular triangular system, 2 pseudo-rank beyond the solve's rank (the per-problem -7).

batched_check(h::Handle, rc::Integer) = (rc == 0 || rc == 1 || check(h, rc); rc)

"""    gradient_batched_hip(h, n, prob0, count) -> G (n×count): J' rx of every problem of the range (src/enlsip_functions.jl:2690)"""
function gradient_batched_hip(h::Handle, n::Integer, prob0::Integer, count::Integer)
    G = zeros(Float64, n, count)
    GC.@preserve G check(h, ccall((:enlsip_gn_gradient_batched, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}),
                                  h.ptr, prob0, count, G))
    return G
end

"""    jacobian_times_batched_hip(h, m, t_max, P, prob0) -> (JP (m×count), AP (t_max×count)): the line-search products
(src/enlsip_functions.jl:2226-2229) of the directions in the columns of `P` (n×count)"""
function jacobian_times_batched_hip(h::Handle, m::Integer, t_max::Integer, P::Matrix{Float64}, prob0::Integer)
    count = size(P, 2)
    JP = zeros(Float64, m, count); AP = zeros(Float64, max(t_max, 1), count)
    GC.@preserve P JP AP check(h, ccall((:enlsip_gn_jacobian_times_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, prob0, count, P, JP, AP))
    return JP, AP[1:t_max, :]
end

"""    first_lagrange_mult_estimate_batched_hip(h, t_max, prob0, count, grads, diag_scales, ε_rank) -> (Λ, grad_res, status)

first_lagrange_mult_estimate! (src/enlsip_functions.jl:461-508) of every problem of the range.  `grads` (n×count) = nothing: J' rx
of the resident J, rx; `diag_scales` (t_max×count) = nothing: no back-transform."""
function first_lagrange_mult_estimate_batched_hip(h::Handle, t_max::Integer, prob0::Integer, count::Integer,
                                                  grads::Union{Nothing,Matrix{Float64}},
                                                  diag_scales::Union{Nothing,Matrix{Float64}}, ε_rank::Float64)
    Λ = zeros(Float64, max(t_max, 1), count); gres = zeros(Float64, count); st = zeros(Cint, count)
    g = grads === nothing ? C_NULL : pointer(grads)
    ds = diag_scales === nothing ? C_NULL : pointer(diag_scales)
    GC.@preserve grads diag_scales Λ gres st batched_check(h, ccall((:enlsip_gn_first_lagrange_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
        h.ptr, prob0, count, g, ds, ε_rank, Λ, gres, st))
    return Λ[1:t_max, :], gres, st
end

"""    second_lagrange_mult_estimate_batched_hip(h, t_max, prob0, P_gn, diag_scales, ε_rank) -> (Λ, status)

second_lagrange_mult_estimate! (src/enlsip_functions.jl:514-537) of every problem of the range; `P_gn` is n×count."""
function second_lagrange_mult_estimate_batched_hip(h::Handle, t_max::Integer, prob0::Integer, P_gn::Matrix{Float64},
                                                   diag_scales::Union{Nothing,Matrix{Float64}}, ε_rank::Float64)
    count = size(P_gn, 2)
    Λ = zeros(Float64, max(t_max, 1), count); st = zeros(Cint, count)
    ds = diag_scales === nothing ? C_NULL : pointer(diag_scales)
    GC.@preserve P_gn diag_scales Λ st batched_check(h, ccall((:enlsip_gn_second_lagrange_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Cint}),
        h.ptr, prob0, count, P_gn, ds, ε_rank, Λ, st))
    return Λ[1:t_max, :], st
end

"""    consumer_form_hip(h) -> 0 general, 1 wave per problem, -1 none yet: the form of the last batched estimate on `h`"""
function consumer_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_consumer_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

const DIM_HOLD = Int64(-2)      # ENLSIP_GN_DIM_HOLD

"""    sub_search_direction_batched_hip(h, m, n, t_max, prob0, dimA, dimJ2, code) -> (P, b, d, infos, status)

`sub_search_direction` (src/enlsip_functions.jl:116-153, called at :1253) of problems `prob0 .. prob0 + length(code) - 1` on the
resident factors, one call.  `code[j]` = 1 / -1, 0 leaves the problem alone (its columns stay NaN); `dimJ2[j] == DIM_HOLD` stops
after b (:1251) and d (:1156-1163), `dimA[j] == DIM_HOLD` finishes such a held call with `dimJ2[j]`: the three-call flow of
search_direction_analys (:1249-1253) around choose_subspace_dimensions (:1118-1176).  status: 0, 1 dimA, 2 dimJ2 out of range,
3 no held result, 4 code."""
function sub_search_direction_batched_hip(h::Handle, m::Integer, n::Integer, t_max::Integer, prob0::Integer,
                                          dimA::Vector{Int64}, dimJ2::Vector{Int64}, code::Vector{Int64})
    count = length(code)
    (length(dimA) == count && length(dimJ2) == count) || error("dimA, dimJ2 and code must have the same length")
    P = fill(NaN, n, count); b = fill(NaN, max(t_max, 1), count); d = fill(NaN, m, count)
    infos = fill(Info(0, 0, 0, 0, 0, 0), count); st = fill(Cint(-1), count)
    GC.@preserve dimA dimJ2 code P b d infos st batched_check(h, ccall((:enlsip_gn_resolve_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Info}, Ptr{Cint}),
        h.ptr, prob0, count, dimA, dimJ2, code, P, b, d, infos, st))
    return P, b[1:t_max, :], d, infos, st
end

"""    diagR_batched_hip(h, which, stride, prob0, count) -> D (stride×count): diag(F.R) of every problem of the range, zeros past
each problem's own length — what choose_subspace_dimensions reads (src/enlsip_functions.jl:1118-1176)"""
function diagR_batched_hip(h::Handle, which::Integer, stride::Integer, prob0::Integer, count::Integer)
    D = zeros(Float64, max(stride, 1), count)
    GC.@preserve D check(h, ccall((:enlsip_gn_get_diagR_batched, LIB), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Int64),
                                  h.ptr, which, prob0, count, D, max(stride, 1)))
    return D
end

"""    resolve_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last batched re-solve on `h`"""
function resolve_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_resolve_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""    determine_solving_dim_hip(previous_dimR, rankR, predicted_linear_progress, obj_progress, prelin_previous_dim, diagR, y,
                              previous_α, restart) -> newdim

`determine_solving_dim` (src/enlsip_functions.jl:1041-1113, with `gn_previous_step` :909-932 and `subspace_min_previous_step`
:864-904) on host data through the library's host entry point (no handle, no GPU): the routine the batched call below runs on the
device.  `η` is not computed (discarded at :1150, :1169).  Throws a `BoundsError` where the reference does."""
function determine_solving_dim_hip(previous_dimR::Integer, rankR::Integer, predicted_linear_progress::Float64, obj_progress::Float64,
                                   prelin_previous_dim::Float64, diagR::Vector{Float64}, y::Vector{Float64}, previous_α::Float64,
                                   restart::Bool)
    (length(diagR) >= rankR && length(y) >= rankR) || error("diagR and y need rankR entries")
    nd = Ref{Int64}(0)
    rc = GC.@preserve diagR y ccall((:enlsip_gn_determine_solving_dim, LIB), Cint,
        (Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Ref{Int64}),
        previous_dimR, rankR, predicted_linear_progress, obj_progress, prelin_previous_dim, diagR, y, previous_α, Int64(restart), nd)
    rc == 5 && throw(BoundsError(y, previous_dimR))
    rc == 0 || error("enlsip_gn_determine_solving_dim returned $rc")
    return Int(nd[])
end

"""what `choose_subspace_dimensions` (src/enlsip_functions.jl:1118-1176) reads of `previous_iter`: enlsip_gn_subspace_prev"""
struct SubspacePrev
    previous_dimA::Int64            # :1144  abs(previous_iter.dimA) + t - previous_iter.t
    previous_dimJ2::Int64           # :1165  abs(previous_iter.dimJ2) + previous_iter.t - t
    restart::Int64                  # current_iter.restart
    previous_alpha::Float64         # previous_iter.α
    constraint_progress::Float64    # :1147  dot(prev.cx, prev.cx) - active_cx_sum
    residual_progress::Float64      # :1168  dot(prev.rx, prev.rx) - rx_sum
end

"""    subspace_direction_batched_hip(h, m, n, t_max, prob0, prev, take) -> (P, b, d, infos, status)

The subspace branch of `search_direction_analys` (src/enlsip_functions.jl:1249-1253, code = -1) for problems
`prob0 .. prob0 + length(prev) - 1` of the resident batch in ONE call: b (:1251), `choose_subspace_dimensions` (:1118-1176) on the
device — dimA from b and diag(F_L11.R), d (:1156-1163), dimJ2 from d and diag(F_J2.R), the max with the previous dimensions
(:1171-1174) — and `sub_search_direction` (:1253) with the chosen pair, which `infos[j].dimA / .dimJ2` carry.  `take[j] == 0`
leaves the problem alone.  status: 0; 1 / 2 the final dimA / dimJ2 is out of range (b, d written, no p); 5 the reference would
throw a BoundsError (nothing written)."""
function subspace_direction_batched_hip(h::Handle, m::Integer, n::Integer, t_max::Integer, prob0::Integer, prev::Vector{SubspacePrev},
                                        take::Union{Nothing,Vector{Int64}} = nothing)
    count = length(prev)
    (take === nothing || length(take) == count) || error("take must have one entry per problem")
    P = fill(NaN, n, count); b = fill(NaN, max(t_max, 1), count); d = fill(NaN, m, count)
    infos = fill(Info(0, 0, 0, 0, 0, 0), count); st = fill(Cint(-1), count)
    tk = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve prev take P b d infos st batched_check(h, @ccall LIB.enlsip_gn_subspace_direction_batched(
        h.ptr::Ptr{Cvoid}, prob0::Int64, count::Int64, tk::Ptr{Int64}, prev::Ptr{SubspacePrev}, P::Ptr{Float64}, b::Ptr{Float64},
        d::Ptr{Float64}, infos::Ptr{Info}, st::Ptr{Cint})::Cint)
    return P, b[1:t_max, :], d, infos, st
end

"""    subspace_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last one-call subspace direction"""
function subspace_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_subspace_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""    check_constraint_deletion_hip(q, λ, scaling, diag_scale, grad_res) -> s

`check_constraint_deletion` (src/enlsip_functions.jl:574-603) on host data through the library's host entry point (no handle, no
GPU): the routine the batched call below runs on the device.  `t = length(λ)`; 0 = no constraint is deleted."""
function check_constraint_deletion_hip(q::Integer, λ::Vector{Float64}, scaling::Bool, diag_scale::Vector{Float64}, grad_res::Float64)
    t = length(λ)
    length(diag_scale) >= t || error("diag_scale needs one entry per multiplier")
    s = Ref{Int64}(0)
    rc = GC.@preserve λ diag_scale ccall((:enlsip_gn_check_constraint_deletion, LIB), Cint,
        (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Cint, Float64, Ref{Int64}), q, t, λ, diag_scale, Cint(scaling), grad_res, s)
    rc == 0 || error("enlsip_gn_check_constraint_deletion returned $rc")
    return Int(s[])
end

"""    delete_constraints_batched_dev_hip(h, B, n, t_max, t, q, take, scaling, dλ, ddiag_scale, dgrad_res, dAt, ldat, strideAt, dcx,
                                       dsaved) -> s

The deletion test (src/enlsip_functions.jl:574-603) of every taken problem on DEVICE buffers and, where it names row `s[k]`, its
removal from `C.A'`, `C.cx`, `C.diag_scale` and `λ` in place (:708-719, :748-756, :776-785), the removed record going to `dsaved`
(n + 3 per problem, `C_NULL` when no undo follows).  `t`, `q` and `take` (`nothing`: all) are host arrays; `dgrad_res == C_NULL` is
`grad_res = 0.0`, the second-order test (:747 / :775).  `s` is 1-based, 0 = nothing; the caller decrements `t` and edits `W`."""
function delete_constraints_batched_dev_hip(h::Handle, B::Integer, n::Integer, t_max::Integer, t::Vector{Int64}, q::Vector{Int64},
                                            take::Union{Nothing,Vector{Int64}}, scaling::Bool, dλ::Ptr{Float64},
                                            ddiag_scale::Ptr{Float64}, dgrad_res::Ptr{Float64}, dAt::Ptr{Float64}, ldat::Integer,
                                            strideAt::Integer, dcx::Ptr{Float64}, dsaved::Ptr{Float64})
    (length(t) == B && length(q) == B && (take === nothing || length(take) == B)) || error("t, q and take need B entries")
    s = zeros(Int64, B)
    tk = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve t q take s check(h, ccall((:enlsip_gn_delete_constraints_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
        h.ptr, B, n, t_max, t, q, tk, Cint(scaling), dλ, ddiag_scale, dgrad_res, dAt, ldat, strideAt, dcx, dsaved, s))
    return s
end

"""    restore_constraints_batched_dev_hip(h, B, n, t_max, t, s, dλ, ddiag_scale, dAt, ldat, strideAt, dcx, dsaved)

The undo of a first-order deletion (src/enlsip_functions.jl:731-739) for the problems with `s[k] != 0`, in place on DEVICE buffers:
the exact inverse of `delete_constraints_batched_dev_hip`, `t[k]` being the count after the deletion.  The feasibility rule
(:728-729) stays with the caller."""
function restore_constraints_batched_dev_hip(h::Handle, B::Integer, n::Integer, t_max::Integer, t::Vector{Int64}, s::Vector{Int64},
                                             dλ::Ptr{Float64}, ddiag_scale::Ptr{Float64}, dAt::Ptr{Float64}, ldat::Integer,
                                             strideAt::Integer, dcx::Ptr{Float64}, dsaved::Ptr{Float64})
    (length(t) == B && length(s) == B) || error("t and s need B entries")
    GC.@preserve t s check(h, ccall((:enlsip_gn_restore_constraints_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64,
         Ptr{Float64}, Ptr{Float64}),
        h.ptr, B, n, t_max, t, s, dλ, ddiag_scale, dAt, ldat, strideAt, dcx, dsaved))
    return nothing
end

"""    deletion_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last delete / restore call on `h`"""
function deletion_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_deletion_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""    evaluate_violated_constraints_hip(l, n, q, t, active, inactive, cx, index_α_upp) -> (t, added, status)

`evaluate_violated_constraints` (src/enlsip_functions.jl:608-650) on host data through the library's host entry point (no handle,
no GPU): the routine the batched call below runs on the device.  `active` and `inactive` hold `l` entries each (1-based, the
first `t` / `l - t` used, 0 behind) and are edited in place.  `status == 1`: the reference would repeat a swap pass for ever; the
lists are left in that unchanged state.  `status == 2`: the pass cap `(l+1)^2` (never observed)."""
function evaluate_violated_constraints_hip(l::Integer, n::Integer, q::Integer, t::Integer, active::Vector{Int64},
                                           inactive::Vector{Int64}, cx::Vector{Float64}, index_α_upp::Integer)
    (length(active) == l && length(inactive) == l && length(cx) == l) || error("active, inactive and cx need l entries")
    tt = Ref{Int64}(t); added = Ref{Int64}(0); status = Ref{Int64}(0)
    rc = GC.@preserve active inactive cx ccall((:enlsip_gn_evaluate_violated_constraints, LIB), Cint,
        (Int64, Int64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ref{Int64}, Ref{Int64}),
        l, n, q, tt, active, inactive, cx, index_α_upp, added, status)
    rc == 0 || error("enlsip_gn_evaluate_violated_constraints returned $rc")
    return Int(tt[]), added[] != 0, Int(status[])
end

"""    gather_active_constraints_hip(active, t, A, cx, scaling) -> (At, cx_active, diag_scale)

`active_C.A = A[active, :]`, `active_C.cx = cx[active]` (src/enlsip_functions.jl:2854-2855) and `evaluate_scaling!`
(src/structures.jl:160-178) on host data through the library's host entry point: `At` is the `n x t` matrix `A'` of the solve."""
function gather_active_constraints_hip(active::Vector{Int64}, t::Integer, A::Matrix{Float64}, cx::Vector{Float64}, scaling::Bool)
    l, n = size(A)
    (length(cx) == l && length(active) >= t) || error("cx needs l entries and active t")
    At = zeros(n, t); ca = zeros(t); ds = zeros(t)
    rc = GC.@preserve active A cx At ca ds ccall((:enlsip_gn_gather_active_constraints, LIB), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
        l, n, t, active, A, max(l, 1), cx, Cint(scaling), At, max(n, 1), ca, ds)
    rc == 0 || error("enlsip_gn_gather_active_constraints returned $rc")
    return At, ca, ds
end

"""    add_constraints_batched_dev_hip(h, B, n, l, t_max, q, t, active, inactive, index_α_upp, take, scaling, dA, lda, strideA,
                                    dcx_all, dAt, ldat, strideAt, dcx, ddiag_scale) -> (added, status)

The walk above for every problem with `take[k] == 1` on the DEVICE buffer `dcx_all`, then (also for `take[k] == 2`) the padded
slot of the ragged solve gathered from `dA` / `dcx_all` into `dAt`, `dcx`, `ddiag_scale`.  `q`, `t`, `index_α_upp`, `take`
(`nothing`: 1 everywhere) are host vectors of `B` entries, `active` / `inactive` host matrices `l x B` (one column per problem);
`t` and the lists of the walked problems are updated in place."""
function add_constraints_batched_dev_hip(h::Handle, B::Integer, n::Integer, l::Integer, t_max::Integer, q::Vector{Int64},
                                         t::Vector{Int64}, active::Matrix{Int64}, inactive::Matrix{Int64},
                                         index_α_upp::Vector{Int64}, take::Union{Nothing,Vector{Int64}}, scaling::Bool,
                                         dA::Ptr{Float64}, lda::Integer, strideA::Integer, dcx_all::Ptr{Float64}, dAt::Ptr{Float64},
                                         ldat::Integer, strideAt::Integer, dcx::Ptr{Float64}, ddiag_scale::Ptr{Float64})
    (length(q) == B && length(t) == B && length(index_α_upp) == B && (take === nothing || length(take) == B)) ||
        error("q, t, index_α_upp and take need B entries")
    (size(active) == (l, B) && size(inactive) == (l, B)) || error("active and inactive are l x B")
    added = zeros(Int64, B); status = zeros(Int64, B)
    tk = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve q t active inactive index_α_upp take added status check(h, ccall((:enlsip_gn_add_constraints_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint,
         Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
        h.ptr, B, n, l, t_max, q, t, active, inactive, index_α_upp, tk, Cint(scaling), dA, lda, strideA, dcx_all, dAt, ldat,
        strideAt, dcx, ddiag_scale, added, status))
    return added, status
end

"""    addition_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last add_constraints call on `h`"""
function addition_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_addition_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""what `check_termination_criteria` (src/enlsip_functions.jl:2399-2517) reads of one problem's host records: enlsip_gn_term_state"""
struct TermState
    restart::Int64                  # :2425  iter.restart (0 / 1)
    code::Int64                     # :2425  iter.code
    del::Int64                      # :2430  iter.del (0 / 1)
    grad_res::Float64               # :2430  iter.grad_res
    nb_iter::Int64                  # :2492  nb_iter
    nb_newton_steps::Int64          # :2500  iter.nb_newton_steps
    error_code::Int64               # :2496  error_code of search_direction_analys
    psi_error::Int64                # :2503  Ψ_error of compute_steplength
    delta_time::Float64             # :2511  Δ_time
    q::Int64                        # :2437  W.q
    t::Int64                        # :2431  W.t
    l::Int64                        # :2431  W.l
    dimJ2::Int64                    # :2448  iter.dimJ2
    psi0::Float64                   # :2279  psi0 of compute_steplength (enters progress only)
end

"""max_iter and the four tolerances of one call: enlsip_gn_term_tol"""
struct TermTol
    max_iter::Int64                 # :2492
    eps_abs::Float64                # :2456  ε_abs
    eps_rel::Float64                # :2430  ε_rel
    eps_x::Float64                  # :2460  ε_x
    eps_c::Float64                  # :2430  ε_c
end

"""the scalars the device forms per problem: enlsip_gn_term_sums"""
struct TermSums
    rx_sum::Float64                 # :2828  dot(rx, rx)
    grad_nrm::Float64               # :2430  norm(∇fx)
    p_nrm::Float64                  # :2422  norm(iter.p)
    active_cx_nrm::Float64          # :2430  norm(active_C.cx)
    n_inactive_nonpos::Int64        # :2434  inactive cx that are not > 0
    n_inactive_le0::Int64           # :2475  inactive cx that are <= 0
    sigma_min::Float64              # :559   σ_min
    lambda_abs_max::Float64         # :554   λ_abs_max
    d1_sq::Float64                  # :2452  dot(d1, d1)
    x_diff::Float64                 # :2449  norm(prev_iter.x - x)
    x_nrm::Float64                  # :2460  norm(x)
    Atcx_nrm::Float64               # :2488  norm(transpose(active_C.A) * active_C.cx)
    active_penalty_sum::Float64     # :2489  dot(w[active], w[active])
    whsum::Float64                  # :2279  sum of w[active] .* cx_new[active].^2
    progress::Float64               # :2280  2 psi0 - rx_sum - whsum
end

"""    minmax_lagrangian_mult_hip(λ, q, t, diag_scale, scaling) -> (σ_min, λ_abs_max)

`minmax_lagrangian_mult` (src/enlsip_functions.jl:540-564) on host data through the library's host entry point (no handle, no
GPU): the routine the batched call below runs on the device.  A NaN among the `t` multipliers makes `λ_abs_max` NaN."""
function minmax_lagrangian_mult_hip(λ::Vector{Float64}, q::Integer, t::Integer, diag_scale::Vector{Float64}, scaling::Bool)
    (t <= q || (length(λ) >= t && length(diag_scale) >= t)) || error("λ and diag_scale need t entries")
    smin = Ref{Float64}(0.0); lmax = Ref{Float64}(0.0)
    rc = GC.@preserve λ diag_scale ccall((:enlsip_gn_minmax_lagrangian_mult, LIB), Cint,
        (Int64, Int64, Ptr{Float64}, Ptr{Float64}, Cint, Ref{Float64}, Ref{Float64}), q, t, λ, diag_scale, Cint(scaling), smin, lmax)
    rc == 0 || error("enlsip_gn_minmax_lagrangian_mult returned $rc")
    return smin[], lmax[]
end

"""    check_termination_criteria_hip(state, sums, tol) -> exit_code

The decision of `check_termination_criteria` (src/enlsip_functions.jl:2420-2516) on scalars, through the library's host entry
point (no handle, no GPU)."""
function check_termination_criteria_hip(state::TermState, sums::TermSums, tol::TermTol)
    code = Ref{Int64}(0)
    rc = @ccall LIB.enlsip_gn_check_termination_criteria(Ref(state)::Ptr{TermState}, Ref(sums)::Ptr{TermSums},
                                                         Ref(tol)::Ptr{TermTol}, code::Ptr{Int64})::Cint
    rc == 0 || error("enlsip_gn_check_termination_criteria returned $rc")
    return Int(code[])
end

"""    termination_sums_hip(state, active, inactive, J, rx, cx_all, x, x_prev, p, d_gn, λ, cx_active, diag_scale, At, w, scaling)
        -> (sums, ∇fx)

The scalars of the termination test from host arrays of one problem, in the summation orders of the kernels (enlsip_gn_termination_sums);
`q`, `t`, `dimJ2` and `psi0` are read from `state`.  `At` is the `n x t` matrix of the OLD active slot."""
function termination_sums_hip(state::TermState, active::Vector{Int64}, inactive::Vector{Int64}, J::Matrix{Float64},
                              rx::Vector{Float64}, cx_all::Vector{Float64}, x::Vector{Float64}, x_prev::Vector{Float64},
                              p::Vector{Float64}, d_gn::Vector{Float64}, λ::Vector{Float64}, cx_active::Vector{Float64},
                              diag_scale::Vector{Float64}, At::Matrix{Float64}, w::Vector{Float64}, scaling::Bool)
    m, n = size(J)
    l = length(cx_all)
    sums = Ref(TermSums(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)); g = zeros(n)
    none = Ptr{Float64}(C_NULL)
    rc = GC.@preserve active inactive J rx cx_all x x_prev p d_gn λ cx_active diag_scale At w g @ccall LIB.enlsip_gn_termination_sums(
        m::Int64, n::Int64, l::Int64, state.t::Int64, state.q::Int64, state.dimJ2::Int64, state.psi0::Float64,
        pointer(active)::Ptr{Int64}, pointer(inactive)::Ptr{Int64}, pointer(J)::Ptr{Float64}, max(m, 1)::Int64,
        pointer(rx)::Ptr{Float64}, pointer(cx_all)::Ptr{Float64}, pointer(x)::Ptr{Float64}, pointer(x_prev)::Ptr{Float64},
        pointer(p)::Ptr{Float64}, pointer(d_gn)::Ptr{Float64}, pointer(λ)::Ptr{Float64}, pointer(cx_active)::Ptr{Float64},
        pointer(diag_scale)::Ptr{Float64}, pointer(At)::Ptr{Float64}, max(n, 1)::Int64, pointer(w)::Ptr{Float64},
        Cint(scaling)::Cint, none::Ptr{Float64}, none::Ptr{Float64}, pointer(g)::Ptr{Float64}, sums::Ptr{TermSums})::Cint
    rc == 0 || error("enlsip_gn_termination_sums returned $rc")
    return sums[], g
end

"""    termination_batched_dev_hip(h, m, n, l, t_max, states, tol, active, inactive, take, scaling, dJ, ldj, strideJ, drx, dcx_all,
                                dx, dx_prev, dp, dd_gn, dλ, dcx_active, ddiag_scale, dAt, ldat, strideAt, dw, dgrad)
        -> (sums, exit_code)

What stands between `new_point!` and `evaluate_violated_constraints` (src/enlsip_functions.jl:2828-2839) for `B = length(states)`
problems on DEVICE buffers in one call: `∇fx = J' rx` into `dgrad`, `rx_sum`, `minmax_lagrangian_mult` and every norm and count
`check_termination_criteria` reads, then the decision on the host.  `active` / `inactive`: host matrices `l x B` (one column per
problem, 0 behind the used part); `take` (`nothing`: all): `take[k] == 0` leaves problem `k` alone.  The slot (`dλ`, `dcx_active`,
`ddiag_scale`, `dAt`) is the OLD active slot in the padded ragged layout.  `exit_code .== 0` is the take mask of the next
iteration's batched calls."""
function termination_batched_dev_hip(h::Handle, m::Integer, n::Integer, l::Integer, t_max::Integer, states::Vector{TermState},
                                     tol::TermTol, active::Matrix{Int64}, inactive::Matrix{Int64},
                                     take::Union{Nothing,Vector{Int64}}, scaling::Bool, dJ::Ptr{Float64}, ldj::Integer,
                                     strideJ::Integer, drx::Ptr{Float64}, dcx_all::Ptr{Float64}, dx::Ptr{Float64},
                                     dx_prev::Ptr{Float64}, dp::Ptr{Float64}, dd_gn::Ptr{Float64}, dλ::Ptr{Float64},
                                     dcx_active::Ptr{Float64}, ddiag_scale::Ptr{Float64}, dAt::Ptr{Float64}, ldat::Integer,
                                     strideAt::Integer, dw::Ptr{Float64}, dgrad::Ptr{Float64})
    B = length(states)
    (take === nothing || length(take) == B) || error("take must have one entry per problem")
    (size(active) == (l, B) && size(inactive) == (l, B)) || error("active and inactive are l x B")
    sums = fill(TermSums(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), B); codes = zeros(Int64, B)
    tk = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve states active inactive take sums codes check(h, @ccall LIB.enlsip_gn_termination_batched_dev(
        h.ptr::Ptr{Cvoid}, B::Int64, m::Int64, n::Int64, l::Int64, t_max::Int64, pointer(states)::Ptr{TermState},
        Ref(tol)::Ptr{TermTol}, pointer(active)::Ptr{Int64}, pointer(inactive)::Ptr{Int64}, tk::Ptr{Int64}, Cint(scaling)::Cint,
        dJ::Ptr{Float64}, ldj::Int64, strideJ::Int64, drx::Ptr{Float64}, dcx_all::Ptr{Float64}, dx::Ptr{Float64},
        dx_prev::Ptr{Float64}, dp::Ptr{Float64}, dd_gn::Ptr{Float64}, dλ::Ptr{Float64}, dcx_active::Ptr{Float64},
        ddiag_scale::Ptr{Float64}, dAt::Ptr{Float64}, ldat::Int64, strideAt::Int64, dw::Ptr{Float64}, dgrad::Ptr{Float64},
        pointer(sums)::Ptr{TermSums}, pointer(codes)::Ptr{Int64})::Cint)
    return sums, codes
end

"""    termination_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last termination call on `h`"""
function termination_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_termination_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""what `check_gn_direction` (src/enlsip_functions.jl:943-1030) and the norms of `search_direction_analys` (:1222-1231) read of one
problem's host records: enlsip_gn_dir_state"""
struct DirState
    iter_number::Int64              # :981   iter_number
    restart::Int64                  # :974   current_iter.restart (0 / 1)
    add::Int64                      # :983   current_iter.add (0 / 1)
    del::Int64                      # :983   current_iter.del (0 / 1)
    q::Int64                        # :998   W.q
    t::Int64                        # :998   W.t
    l::Int64                        # :1007  W.l
    rankA::Int64                    # :1015  current_iter.rankA
    dimA::Int64                     # :1222  current_iter.dimA
    dimJ2::Int64                    # :1228  current_iter.dimJ2
    prev_code::Int64                # :974   previous_iter.code
    prev_dimJ2::Int64               # :1230  previous_iter.dimJ2
    prev_t::Int64                   # :1230  previous_iter.t
    prev_beta::Float64              # :984   previous_iter.β
    prev_progress::Float64          # :985   previous_iter.progress
    prev_predicted_reduction::Float64      # :985   previous_iter.predicted_reduction
    prev_alpha::Float64             # :1020  previous_iter.α
end

"""the scalars the device forms per problem: enlsip_gn_dir_sums"""
struct DirSums
    b1_sq::Float64                  # :1222  dot(b1, b1)
    d_sq::Float64                   # :1227  dot(d_gn, d_gn)
    d1_sq::Float64                  # :1228  dot(d1, d1)
    d1_asprev_sq::Float64           # :1231  the same over d_gn[1:k_prev]
    active_c_sum::Float64           # :1013  active_cx_sum
    n_lm_ge::Int64                  # :1004  multipliers of q+1..t with λ_i * rows_i >= -sqrt(eps)
    n_lm_neg::Int64                 # :1004  multipliers of q+1..t below 0
    n_inactive_lt_delta::Int64      # :1009  inactive cx below δ
end

"""    check_gn_direction_hip(state, sums, m, n) -> (method_code, β)

The decision of `check_gn_direction` (src/enlsip_functions.jl:943-1030) on scalars, through the library's host entry point (no
handle, no GPU)."""
function check_gn_direction_hip(state::DirState, sums::DirSums, m::Integer, n::Integer)
    code = Ref{Int64}(0); β = Ref{Float64}(0.0)
    rc = @ccall LIB.enlsip_gn_check_gn_direction(Ref(state)::Ptr{DirState}, Ref(sums)::Ptr{DirSums}, m::Int64, n::Int64,
                                                 code::Ptr{Int64}, β::Ptr{Float64})::Cint
    rc == 0 || error("enlsip_gn_check_gn_direction returned $rc")
    return Int(code[]), β[]
end

"""    direction_sums_hip(state, m, n, active, inactive, b, d, λ, diag_scale, cx_all, scaling) -> (sums, status)

The scalars of the direction check from host arrays of one problem, in the summation order of the kernels
(enlsip_gn_direction_sums).  `status == 1`: the reference would index `d_gn` past its end (:1231) and `sums` is all zero."""
function direction_sums_hip(state::DirState, m::Integer, n::Integer, active::Vector{Int64}, inactive::Vector{Int64},
                            b::Vector{Float64}, d::Vector{Float64}, λ::Vector{Float64}, diag_scale::Vector{Float64},
                            cx_all::Vector{Float64}, scaling::Bool)
    sums = Ref(DirSums(0, 0, 0, 0, 0, 0, 0, 0)); status = Ref{Int64}(0); sc = Cint(scaling)
    rc = GC.@preserve active inactive b d λ diag_scale cx_all @ccall LIB.enlsip_gn_direction_sums(
        m::Int64, n::Int64, length(cx_all)::Int64, Ref(state)::Ptr{DirState}, pointer(active)::Ptr{Int64},
        pointer(inactive)::Ptr{Int64}, pointer(b)::Ptr{Float64}, pointer(d)::Ptr{Float64}, pointer(λ)::Ptr{Float64},
        pointer(diag_scale)::Ptr{Float64}, pointer(cx_all)::Ptr{Float64}, sc::Cint, sums::Ptr{DirSums},
        status::Ptr{Int64})::Cint
    rc == 0 || error("enlsip_gn_direction_sums returned $rc")
    return sums[], Int(status[])
end

"""    direction_check_batched_dev_hip(h, m, n, l, t_max, states, active, inactive, take, scaling, db, dd, dλ, ddiag_scale, dcx_all)
        -> (sums, method_code, β, status)

`search_direction_analys` (src/enlsip_functions.jl:1191-1291) up to its branch for `B = length(states)` problems on DEVICE buffers
in one call: the norms of :1222-1231 and `check_gn_direction`.  `db`, `dd`, `dλ`, `ddiag_scale` are where the solve and the
multiplier calls left them; `active` / `inactive`: host matrices `l x B`; `take` (`nothing`: all): `take[k] == 0` leaves problem
`k` alone.  `method_code .== -1` is the take of `subspace_direction_batched_dev`, `method_code .== 2` that of the batched Newton
direction.  `status[k] == 1`: the reference throws at :1231, no code; `2`: a prefix of `d_gn` reaches past `n - rankA`
(`d_gn_prefix` would assert)."""
function direction_check_batched_dev_hip(h::Handle, m::Integer, n::Integer, l::Integer, t_max::Integer, states::Vector{DirState},
                                         active::Matrix{Int64}, inactive::Matrix{Int64}, take::Union{Nothing,Vector{Int64}},
                                         scaling::Bool, db::Ptr{Float64}, dd::Ptr{Float64}, dλ::Ptr{Float64},
                                         ddiag_scale::Ptr{Float64}, dcx_all::Ptr{Float64})
    B = length(states)
    (take === nothing || length(take) == B) || error("take must have one entry per problem")
    (size(active) == (l, B) && size(inactive) == (l, B)) || error("active and inactive are l x B")
    sums = fill(DirSums(0, 0, 0, 0, 0, 0, 0, 0), B); codes = zeros(Int64, B); β = fill(NaN, B); status = fill(Int64(-1), B)
    tk = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take); sc = Cint(scaling)
    GC.@preserve states active inactive take sums codes β status check(h, @ccall LIB.enlsip_gn_direction_check_batched_dev(
        h.ptr::Ptr{Cvoid}, B::Int64, m::Int64, n::Int64, l::Int64, t_max::Int64, pointer(states)::Ptr{DirState},
        pointer(active)::Ptr{Int64}, pointer(inactive)::Ptr{Int64}, tk::Ptr{Int64}, sc::Cint, db::Ptr{Float64},
        dd::Ptr{Float64}, dλ::Ptr{Float64}, ddiag_scale::Ptr{Float64}, dcx_all::Ptr{Float64}, pointer(sums)::Ptr{DirSums},
        pointer(codes)::Ptr{Int64}, pointer(β)::Ptr{Float64}, pointer(status)::Ptr{Int64})::Cint)
    return sums, codes, β, status
end

"""    direction_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last direction check on `h`"""
function direction_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, @ccall LIB.enlsip_gn_get_direction_form(h.ptr::Ptr{Cvoid}, f::Ptr{Cint})::Cint)
    return Int(f[])
end

"""    hessian_points_hip(x, pair0, npairs) -> X (n × 4 × npairs)

The stencil points of `hessian_res!` / `hessian_cons!` (src/enlsip_functions.jl:259-265) for the pairs `pair0 .. pair0 + npairs - 1`
(0-based pair index `P = k (k + 1) / 2 + j`, the loop order of :255 with 0-based `j ≤ k`), through the library's host entry point
(no handle, no GPU): `X[:, s, q]` is `x_work` before evaluation `f_s` of pair `q`, bit for bit."""
function hessian_points_hip(x::Vector{Float64}, pair0::Integer, npairs::Integer)
    n = length(x)
    X = zeros(n, 4, max(npairs, 0))
    rc = GC.@preserve x X @ccall LIB.enlsip_gn_hessian_points(n::Int64, pair0::Int64, npairs::Int64, pointer(x)::Ptr{Float64},
                                                               pointer(X)::Ptr{Float64})::Cint
    rc == 0 || error("enlsip_gn_hessian_points returned $rc")
    return X
end

"""    hessian_points_batched_dev_hip(h, B, n, pair0, npairs, dx, dX)

The same for `B` problems on DEVICE buffers: `dx` (`n × B`) in, `dX` (`n × 4 × npairs × B`) out, in one launch."""
function hessian_points_batched_dev_hip(h::Handle, B::Integer, n::Integer, pair0::Integer, npairs::Integer, dx::Ptr{Float64},
                                        dX::Ptr{Float64})
    check(h, @ccall LIB.enlsip_gn_hessian_points_batched_dev(h.ptr::Ptr{Cvoid}, B::Int64, n::Int64, pair0::Int64, npairs::Int64,
                                                             dx::Ptr{Float64}, dX::Ptr{Float64})::Cint)
    return nothing
end

"""    hessian_sums_hip!(Γ, x, F, rx, G, λ, active, t, pair0) -> Γ

`Γ[k, j] = Γ[j, k] = r - c` (src/enlsip_functions.jl:268-272, :317-322, :393) for the pairs `pair0 .. pair0 + size(F, 3) - 1` from
the evaluations `F` (`m × 4 × npairs`, the residuals) and `G` (`l × 4 × npairs`, all constraints) at the points of
`hessian_points_hip`, through the library's host entry point.  The sums are taken in the library's documented order (64 strided
partials and a butterfly), not left to right.  Only the entries of the pairs in the range are written."""
function hessian_sums_hip!(Γ::Matrix{Float64}, x::Vector{Float64}, F::Array{Float64,3}, rx::Vector{Float64}, G::Array{Float64,3},
                           λ::Vector{Float64}, active::Vector{Int64}, t::Integer, pair0::Integer)
    n = length(x); m = length(rx); l = size(G, 1); npairs = size(F, 3); ldg = size(Γ, 1)
    (size(F, 1) == m && size(F, 2) == 4 && size(G, 2) == 4 && size(G, 3) == npairs) || error("F is m x 4 x npairs, G l x 4 x npairs")
    (size(Γ, 2) == n && ldg >= n && length(λ) >= t && length(active) >= t) || error("Γ has n columns; λ and active need t entries")
    rc = GC.@preserve Γ x F rx G λ active @ccall LIB.enlsip_gn_hessian_sums(
        m::Int64, n::Int64, l::Int64, t::Int64, pair0::Int64, npairs::Int64, pointer(active)::Ptr{Int64}, pointer(x)::Ptr{Float64},
        pointer(F)::Ptr{Float64}, pointer(rx)::Ptr{Float64}, pointer(G)::Ptr{Float64}, pointer(λ)::Ptr{Float64},
        pointer(Γ)::Ptr{Float64}, ldg::Int64)::Cint
    rc == 0 || error("enlsip_gn_hessian_sums returned $rc")
    return Γ
end

"""    hessian_sums_batched_dev_hip(h, m, n, l, t_max, pair0, npairs, t, active, slot, dx, dF, drx, dG, dλ, dΓ, ldg, strideΓ)

The same for `B = length(t)` problems on DEVICE buffers in one launch: `Γ` of problem `k` is written column-major at
`dΓ + slot[k] * strideΓ`, where the batched Newton direction reads it (`slot === nothing`: slot `k`; `slot[k] < 0` leaves problem
`k` alone).  `active`: host matrix `l × B`, 1-based, 0 behind the used part."""
function hessian_sums_batched_dev_hip(h::Handle, m::Integer, n::Integer, l::Integer, t_max::Integer, pair0::Integer, npairs::Integer,
                                      t::Vector{Int64}, active::Matrix{Int64}, slot::Union{Nothing,Vector{Int64}},
                                      dx::Ptr{Float64}, dF::Ptr{Float64}, drx::Ptr{Float64}, dG::Ptr{Float64}, dλ::Ptr{Float64},
                                      dΓ::Ptr{Float64}, ldg::Integer, strideΓ::Integer)
    B = length(t)
    size(active) == (l, B) || error("active is l x B")
    (slot === nothing || length(slot) == B) || error("slot must have one entry per problem")
    sl = slot === nothing ? Ptr{Int64}(C_NULL) : pointer(slot)
    GC.@preserve t active slot check(h, @ccall LIB.enlsip_gn_hessian_sums_batched_dev(
        h.ptr::Ptr{Cvoid}, B::Int64, m::Int64, n::Int64, l::Int64, t_max::Int64, pair0::Int64, npairs::Int64, pointer(t)::Ptr{Int64},
        pointer(active)::Ptr{Int64}, sl::Ptr{Int64}, dx::Ptr{Float64}, dF::Ptr{Float64}, drx::Ptr{Float64}, dG::Ptr{Float64},
        dλ::Ptr{Float64}, dΓ::Ptr{Float64}, ldg::Int64, strideΓ::Int64)::Cint)
    return nothing
end

"""    upper_bound_steplength_hip(inactive, n_inactive, index_del, cx, Ap) -> (α_upp, index_α_upp)

`upper_bound_steplength` (src/enlsip_functions.jl:2149-2178) on host data with `Ap = A * p` already formed, through the library's
host entry point (no handle, no GPU): the routine the batched call below runs on the device.  `inactive` holds 1-based rows (0 =
padding) of which the first `n_inactive` are walked in list order; `l = length(cx)`."""
function upper_bound_steplength_hip(inactive::Vector{Int64}, n_inactive::Integer, index_del::Integer, cx::Vector{Float64},
                                    Ap::Vector{Float64})
    l = length(cx)
    (length(Ap) == l && length(inactive) >= n_inactive) || error("cx and Ap need l entries, inactive n_inactive")
    α = Ref{Float64}(0.0)
    idx = Ref{Int64}(0)
    rc = GC.@preserve inactive cx Ap ccall((:enlsip_gn_upper_bound_steplength, LIB), Cint,
        (Int64, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Int64}),
        l, n_inactive, inactive, index_del, cx, Ap, α, idx)
    rc == 0 || error("enlsip_gn_upper_bound_steplength returned $rc")
    return α[], Int(idx[])
end

"""    linesearch_setup_batched_dev_hip(h, B, m, n, l, dp, dA, lda, strideA, dcx, inactive, n_inactive, index_del, dJp, drx, dAp)
        -> (α_upp, index_α_upp, sums)

The line-search set-up of a batch on DEVICE buffers: `Ap = A * p` with the full constraint Jacobian into `dAp` (:2226-2229),
`upper_bound_steplength` on it (:2149-2178) and, unless `dJp` and `drx` are `C_NULL`, the sums `dot(Jp,Jp)`, `dot(Jp,rx)`,
`dot(rx,rx)` of :1561-1584 / :2269 as the columns of the 3 x B matrix `sums` (`nothing` without them).  `inactive` (l x B, zero
padded: problem k's list is column k), `n_inactive` and `index_del` (`nothing`: 0) are host arrays."""
function linesearch_setup_batched_dev_hip(h::Handle, B::Integer, m::Integer, n::Integer, l::Integer, dp::Ptr{Float64},
                                          dA::Ptr{Float64}, lda::Integer, strideA::Integer, dcx::Ptr{Float64},
                                          inactive::Matrix{Int64}, n_inactive::Vector{Int64},
                                          index_del::Union{Nothing,Vector{Int64}}, dJp::Ptr{Float64}, drx::Ptr{Float64},
                                          dAp::Ptr{Float64})
    (size(inactive) == (l, B) && length(n_inactive) == B && (index_del === nothing || length(index_del) == B)) ||
        error("inactive is l x B, n_inactive and index_del need B entries")
    α = zeros(Float64, B)
    idx = zeros(Int64, B)
    with_sums = dJp != C_NULL && drx != C_NULL
    sums = with_sums ? zeros(Float64, 3, B) : nothing
    psums = with_sums ? pointer(sums) : Ptr{Float64}(C_NULL)
    pdel = index_del === nothing ? Ptr{Int64}(C_NULL) : pointer(index_del)
    GC.@preserve inactive n_inactive index_del α idx sums check(h, ccall((:enlsip_gn_linesearch_setup_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int64},
         Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
        h.ptr, B, m, n, l, dp, dA, lda, strideA, dcx, inactive, n_inactive, pdel, dJp, drx, dAp, α, idx, psums))
    return α, idx, sums
end

"""    linesearch_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last line-search set-up on `h`"""
function linesearch_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_linesearch_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""    penalty_weight_update_hip(w_old, active, t, dimA, norm_code, active_Ap, cx, K, JpJp, Jprx, rxrx) -> (w, dψ0, ψ0, atwa, branch)

`penalty_weight_update` (src/enlsip_functions.jl:1545-1629) with ψ(0) of :2243 and `atwa` of :2268 on host data, through the
library's host entry point (no handle, no GPU): the routine the batched call below runs on the device.  `active_Ap` holds the `t`
entries of `C.A * p`, already divided by `diag_scale` where scaling is on; `K` is the l x 4 matrix whose column ii is `K[ii]` of
the reference and is updated in place; `Jp` and `rx` enter through the three sums of the set-up call."""
function penalty_weight_update_hip(w_old::Vector{Float64}, active::Vector{Int64}, t::Integer, dimA::Integer, norm_code::Integer,
                                   active_Ap::Vector{Float64}, cx::Vector{Float64}, K::Matrix{Float64}, JpJp::Float64,
                                   Jprx::Float64, rxrx::Float64)
    l = length(w_old)
    (length(cx) == l && size(K) == (l, 4) && length(active) >= t && length(active_Ap) >= t) ||
        error("cx needs l entries, K is l x 4, active and active_Ap need t entries")
    w = zeros(Float64, l)
    sc = zeros(Float64, 3)
    br = Ref{Cint}(0)
    rc = GC.@preserve w_old active active_Ap cx K w sc ccall((:enlsip_gn_penalty_weight_update, LIB), Cint,
        (Int64, Int64, Ptr{Int64}, Int64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Float64, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ref{Cint}),
        l, t, active, dimA, norm_code, w_old, active_Ap, cx, JpJp, Jprx, rxrx, K, w, sc, br)
    rc == 0 || error("enlsip_gn_penalty_weight_update returned $rc")
    return w, sc[1], sc[2], sc[3], Int(br[])
end

"""    penalty_weights_batched_dev_hip(h, B, l, t_max, t, dimA, active, take, norm_code, scaling, dw_old, dactive_Ap, ddiag_scale,
                                    dcx, dK, sums, dw) -> (scalars, branch)

`penalty_weight_update` (:2238) for every taken problem of a batch on DEVICE buffers: `dw` (l per problem) and `dK` (4 l per
problem) are written there, the division `active_Ap ./ diag_scale` (:2231-2233) happens inside when `scaling`.  `t`, `dimA`,
`active` (t_max x B, zero padded: problem k's list is column k), `take` (`nothing`: all) and `sums` (3 x B, as the set-up call
returns them) are host arrays.  Returns `scalars` (3 x B: dψ0, ψ0, atwa) and `branch`; both 0 for a problem not taken."""
function penalty_weights_batched_dev_hip(h::Handle, B::Integer, l::Integer, t_max::Integer, t::Vector{Int64}, dimA::Vector{Int64},
                                         active::Matrix{Int64}, take::Union{Nothing,Vector{Int64}}, norm_code::Integer,
                                         scaling::Bool, dw_old::Ptr{Float64}, dactive_Ap::Ptr{Float64},
                                         ddiag_scale::Ptr{Float64}, dcx::Ptr{Float64}, dK::Ptr{Float64}, sums::Matrix{Float64},
                                         dw::Ptr{Float64})
    (size(active) == (t_max, B) && length(t) == B && length(dimA) == B && size(sums) == (3, B) &&
     (take === nothing || length(take) == B)) || error("active is t_max x B, sums 3 x B, t, dimA and take need B entries")
    scalars = zeros(Float64, 3, B)
    branch = zeros(Cint, B)
    ptake = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve t dimA active take sums scalars branch check(h, ccall((:enlsip_gn_penalty_weights_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint, Cint, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
        h.ptr, B, l, t_max, t, dimA, active, ptake, norm_code, scaling ? 1 : 0, dw_old, dactive_Ap, ddiag_scale, dcx, dK, sums, dw,
        scalars, branch))
    return scalars, branch
end

"""    penalty_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last penalty-weight call on `h`"""
function penalty_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_penalty_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

"""    merit_batched_dev_hip(h, B, m, l, t_max, t, active, inactive, n_inactive, take, drx, dcx, dw) -> ψ

The merit function `psi` (:1307-1340) of one evaluated trial point per problem on DEVICE buffers `drx` (m per problem), `dcx` and
`dw` (l per problem).  `t`, `active` (t_max x B), `inactive` (l x B), `n_inactive` and `take` (`nothing`: all) are host arrays."""
function merit_batched_dev_hip(h::Handle, B::Integer, m::Integer, l::Integer, t_max::Integer, t::Vector{Int64},
                               active::Matrix{Int64}, inactive::Matrix{Int64}, n_inactive::Vector{Int64},
                               take::Union{Nothing,Vector{Int64}}, drx::Ptr{Float64}, dcx::Ptr{Float64}, dw::Ptr{Float64})
    (size(active) == (t_max, B) && size(inactive) == (l, B) && length(t) == B && length(n_inactive) == B &&
     (take === nothing || length(take) == B)) || error("active is t_max x B, inactive l x B, t, n_inactive and take need B entries")
    ψ = zeros(Float64, B)
    ptake = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    GC.@preserve t active inactive n_inactive take ψ check(h, ccall((:enlsip_gn_merit_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h.ptr, B, m, l, t_max, t, active, inactive, n_inactive, ptake, drx, dcx, dw, ψ))
    return ψ
end

"""    linesearch_coefficients_hip(active, t, inactive, n_inactive, rx, rx_new, Jp, cx, cx_new, Ap, w, α_k) -> sums

The six dot products v0·v0, v0·v1, v0·v2, v1·v1, v1·v2, v2·v2 of `coefficients_linesearch!` (src/enlsip_functions.jl:1665-1689)
with the scaling of `v1 = [Jp; Ap]` (:1986-1998) on host data, through the library's host entry point (no handle, no GPU).  `Ap` is
the UNSCALED `A * p`; neither `Jp` nor `Ap` is written.  The terms are added in the order residuals, active list, inactive list."""
function linesearch_coefficients_hip(active::Vector{Int64}, t::Integer, inactive::Vector{Int64}, n_inactive::Integer,
                                     rx::Vector{Float64}, rx_new::Vector{Float64}, Jp::Vector{Float64}, cx::Vector{Float64},
                                     cx_new::Vector{Float64}, Ap::Vector{Float64}, w::Vector{Float64}, α_k::Float64)
    m, l = length(rx), length(cx)
    (length(rx_new) == m && length(Jp) == m && length(cx_new) == l && length(Ap) == l && length(w) == l &&
     length(active) >= t && length(inactive) >= n_inactive) || error("rx, rx_new, Jp need m entries, cx, cx_new, Ap, w need l")
    sums = zeros(Float64, 6)
    rc = GC.@preserve active inactive rx rx_new Jp cx cx_new Ap w sums ccall((:enlsip_gn_linesearch_coefficients, LIB), Cint,
        (Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}),
        m, l, t, active, inactive, n_inactive, rx, rx_new, Jp, cx, cx_new, Ap, w, α_k, sums)
    rc == 0 || error("enlsip_gn_linesearch_coefficients returned $rc")
    return sums
end

"""    linesearch_fit_hip(sums, α_k, x_min, α_min, α_max) -> (α_kp1, pk, α_hat, sα, β_hat, sβ, arm)

`minrm` (src/enlsip_functions.jl:1841-1862) on the six sums and the choice of :2023-2026; `arm` 0 Newton–Raphson, 1 one root,
2 two roots."""
function linesearch_fit_hip(sums::Vector{Float64}, α_k::Float64, x_min::Float64, α_min::Float64, α_max::Float64)
    length(sums) == 6 || error("sums needs 6 entries")
    out = zeros(Float64, 6)
    arm = Ref{Cint}(0)
    rc = GC.@preserve sums out ccall((:enlsip_gn_linesearch_fit, LIB), Cint,
        (Ptr{Float64}, Float64, Float64, Float64, Float64, Ptr{Float64}, Ref{Cint}), sums, α_k, x_min, α_min, α_max, out, arm)
    rc == 0 || error("enlsip_gn_linesearch_fit returned $rc")
    return out[1], out[2], out[3], out[4], out[5], out[6], Int(arm[])
end

"""    minrn_hip(x1, y1, x2, y2, x3, y3, α_min, α_max, p_max) -> (α, pα): `minrn` (src/enlsip_functions.jl:1708-1735)"""
function minrn_hip(x1::Float64, y1::Float64, x2::Float64, y2::Float64, x3::Float64, y3::Float64, α_min::Float64, α_max::Float64,
                   p_max::Float64)
    α = Ref{Float64}(0.0)
    pα = Ref{Float64}(0.0)
    rc = ccall((:enlsip_gn_minrn, LIB), Cint,
        (Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Float64, Ref{Float64}, Ref{Float64}),
        x1, y1, x2, y2, x3, y3, α_min, α_max, p_max, α, pα)
    rc == 0 || error("enlsip_gn_minrn returned $rc")
    return α[], pα[]
end

"""    check_reduction_hip(ψ_α, ψ_k, approx_k, η, diff_psi) -> Bool: `check_reduction` (src/enlsip_functions.jl:1870-1886)"""
function check_reduction_hip(ψ_α::Float64, ψ_k::Float64, approx_k::Float64, η::Float64, diff_psi::Float64)
    likely = Ref{Cint}(0)
    rc = ccall((:enlsip_gn_check_reduction, LIB), Cint, (Float64, Float64, Float64, Float64, Float64, Ref{Cint}),
        ψ_α, ψ_k, approx_k, η, diff_psi, likely)
    rc == 0 || error("enlsip_gn_check_reduction returned $rc")
    return likely[] != 0
end

"""    linesearch_fit_batched_dev_hip(h, B, m, l, t_max, t, active, inactive, n_inactive, take, α_k, x_min, α_min, α_max, drx,
                                   drx_new, dJp, dcx, dcx_new, dAp, dw; psi=false) -> (sums, out, arm, ψ_new)

The polynomial fit of the line search for every taken problem of a batch: the six sums on DEVICE buffers (`drx`, `drx_new`, `dJp`
m per problem; `dcx`, `dcx_new`, `dAp`, `dw` l per problem; none is written), then `linesearch_fit_hip`'s routine on the host inside
the same call.  `t`, `active` (t_max x B), `inactive` (l x B), `n_inactive`, `take` (`nothing`: all), `α_k`, `x_min`, `α_min`,
`α_max` are host arrays.  Returns `sums` (6 x B), `out` (6 x B: α_kp1, pk, α_hat, sα, β_hat, sβ), `arm` and, with `psi=true`, ψ of
`(drx_new, dcx_new, dw)` as `merit_batched_dev_hip` returns it (else `nothing`); zeros for a problem not taken."""
function linesearch_fit_batched_dev_hip(h::Handle, B::Integer, m::Integer, l::Integer, t_max::Integer, t::Vector{Int64},
                                        active::Matrix{Int64}, inactive::Matrix{Int64}, n_inactive::Vector{Int64},
                                        take::Union{Nothing,Vector{Int64}}, α_k::Vector{Float64}, x_min::Vector{Float64},
                                        α_min::Vector{Float64}, α_max::Vector{Float64}, drx::Ptr{Float64}, drx_new::Ptr{Float64},
                                        dJp::Ptr{Float64}, dcx::Ptr{Float64}, dcx_new::Ptr{Float64}, dAp::Ptr{Float64},
                                        dw::Ptr{Float64}; psi::Bool=false)
    (size(active) == (t_max, B) && size(inactive) == (l, B) && length(t) == B && length(n_inactive) == B && length(α_k) == B &&
     length(x_min) == B && length(α_min) == B && length(α_max) == B && (take === nothing || length(take) == B)) ||
        error("active is t_max x B, inactive l x B, every other host array needs B entries")
    sums = zeros(Float64, 6, B)
    out = zeros(Float64, 6, B)
    arm = zeros(Cint, B)
    ψ = psi ? zeros(Float64, B) : nothing
    ptake = take === nothing ? Ptr{Int64}(C_NULL) : pointer(take)
    pψ = psi ? pointer(ψ) : Ptr{Float64}(C_NULL)
    GC.@preserve t active inactive n_inactive take α_k x_min α_min α_max sums out arm ψ check(h,
        ccall((:enlsip_gn_linesearch_fit_batched_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}),
        h.ptr, B, m, l, t_max, t, active, inactive, n_inactive, ptake, α_k, x_min, α_min, α_max, drx, drx_new, dJp, dcx, dcx_new,
        dAp, dw, sums, out, arm, pψ))
    return sums, out, arm, ψ
end

"""    newton_search_direction_hip(h, Γ_mat) -> (p, error)

`newton_search_direction` (src/enlsip_functions.jl:348-423) after its two Hessian sums: the caller runs `hessian_res!` /
`hessian_cons!` (:391-394, callback-bound) and passes `Γ_mat = r_mat - c_mat`; the library does :398-421 on the resident
`F_A`, `p1`, `J` of the last solve.  Full-rank working sets only (`t == rankA`); the rank-deficient branch stays in Julia.
"""
function newton_search_direction_hip(h::Handle, Γ_mat::Matrix{Float64})
    n = size(Γ_mat, 1)
    p = zeros(Float64, n)
    bad = Ref{Int64}(0)
    GC.@preserve Γ_mat p check(h, ccall((:enlsip_gn_newton_direction, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ref{Int64}), h.ptr, 0, Γ_mat, n, p, bad))
    return p, bad[] != 0
end

"""    newton_search_direction_batched_hip(h, prob0, Γ, take) -> (P, status)

`newton_search_direction` (src/enlsip_functions.jl:348-423) after its Hessian sums for problems `prob0 .. prob0 + size(Γ, 3) - 1`
of the resident batch, one call: `Γ[:, :, j]` is `r_mat - c_mat` of problem `prob0 + j - 1`; `take[j] == 0` leaves the problem
alone (its column of `P` stays NaN, its status -1) — only the members whose `method_code` is 2 take the step.  status: 0; 1 the
symmetrised W22 is not positive definite (column of zeros: the reference's `error = true`); 2 rank-deficient working set with
t < n (the reference runs out of bounds there)."""
function newton_search_direction_batched_hip(h::Handle, prob0::Integer, Γ::Array{Float64,3},
                                             take::Union{Nothing,Vector{Int64}} = nothing)
    n = size(Γ, 1); count = size(Γ, 3)
    size(Γ, 2) == n || error("Γ must be n×n×count")
    (take === nothing || length(take) == count) || error("take must have one entry per problem")
    P = fill(NaN, n, count); st = fill(Cint(-1), count)
    tk = take === nothing ? C_NULL : pointer(take)
    GC.@preserve Γ take P st batched_check(h, ccall((:enlsip_gn_newton_direction_batched, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Cint}),
        h.ptr, prob0, count, Γ, n, n * n, tk, P, st))
    return P, st
end

"""    newton_form_hip(h) -> 0 general, 1 one wave per problem, -1 none yet: the form of the last batched Newton direction on `h`"""
function newton_form_hip(h::Handle)
    f = Ref{Cint}(0)
    check(h, ccall((:enlsip_gn_get_newton_form, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}), h.ptr, f))
    return Int(f[])
end

# ---- one tall Jacobian, rows sharded over the GPUs of a node (config C4): the library's TSQR collective -------------------------
#
# One Julia process per GPU (Distributed / MPI.jl); every rank creates its Handle on its own device.  Rank 0 obtains the RCCL
# unique id, the caller's own transport carries its 128 bytes to the other ranks (e.g. `MPI.Bcast!(id, 0, comm)` or
# `remotecall_fetch`), then every rank calls `tsqr_init_rccl!` (collective: ncclCommInitRank inside the library) once.
# Afterwards `gn_search_direction_tsqr_hip` is `gn_search_direction` for a Jacobian whose rows live on several GPUs: rank g
# passes DEVICE pointers to its row block of J and rx (e.g. `pointer(::ROCArray)` from AMDGPU.jl) and the replicated C.A', cx;
# every rank gets the same p, ||d||, ranks and pivots back.  The one exchange step is an ncclAllGather of the packed triangles
# (8 n2 (n2 + 1) / 2 bytes per rank) over xGMI, issued by the library on the handle's stream.

"""    tsqr_unique_id() -> Vector{UInt8} (128 bytes; call on rank 0, broadcast with your own transport)"""
function tsqr_unique_id()
    id = zeros(UInt8, 128)
    rc = GC.@preserve id ccall((:enlsip_gn_tsqr_unique_id, LIB), Cint, (Ptr{UInt8},), id)
    rc == 0 || error("enlsip_gn_tsqr_unique_id failed with code $rc (RCCL not loadable?)")
    return id
end

"""    tsqr_init_rccl!(h, id, nranks, rank)  (collective over all ranks; rank is 0-based)"""
function tsqr_init_rccl!(h::Handle, id::Vector{UInt8}, nranks::Integer, rank::Integer)
    length(id) == 128 || error("the RCCL unique id has 128 bytes")
    GC.@preserve id check(h, ccall((:enlsip_gn_tsqr_init_rccl, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint),
                                   h.ptr, id, nranks, rank))
end

"""    gn_search_direction_tsqr_hip(h, dJ, ldj, drx, dAt, dcx, m_loc, n, t, ε_rank) -> (p, d_lead, d_norm, info, jpvtJ2)

Collective.  `dJ`, `drx`: device pointers to this rank's `m_loc` rows of `J` (column-major, leading dimension `ldj`) and `rx`;
`dAt`, `dcx`: device pointers to the replicated `C.A'` (`n×t`, column-major) and `C.cx` (C_NULL when `t == 0`).  Replaces
`JQ1 = J * F_A.Q` … `qr(J2, ColumnNorm())` … `sub_search_direction` (src/enlsip_functions.jl:219-225, :116-153) for that Jacobian;
`d_lead` = leading `n − rankA` entries of `F_J2.Q' d`, `d_norm` = `norm(d_gn)` over all ranks (what :1222-1231 and :2448 consume).
"""
function gn_search_direction_tsqr_hip(h::Handle, dJ::Ptr{Float64}, ldj::Integer, drx::Ptr{Float64}, dAt::Ptr{Float64},
                                      dcx::Ptr{Float64}, m_loc::Integer, n::Integer, t::Integer, ε_rank::Float64)
    p = zeros(Float64, n); dlead = zeros(Float64, n); jJ = zeros(Int64, n)
    dn = Ref{Float64}(0.0)
    info = Ref(Info(0, 0, 0, 0, 0, 0))
    GC.@preserve p dlead jJ check(h, ccall((:enlsip_gn_solve_tsqr, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Float64,
         Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Info}, Ptr{Int64}),
        h.ptr, m_loc, n, t, dJ, ldj, drx, dAt, max(n, 1), dcx, ε_rank, p, dlead, dn, info, jJ))
    (info[].status & 1) != 0 && throw(LinearAlgebra.SingularException(0))
    n2 = n - Int(info[].rankA)
    return p, dlead[1:n2], dn[], info[], jJ[1:n2]
end

# ---- the consumers around the subproblem on a row-sharded J: every rank calls them after `gn_search_direction_tsqr_hip` ------
# The shard (dJ, drx, dAt, dcx) of that call must still be alive and unchanged.  Each call is ONE exchange of n + 3 doubles per
# rank and every rank returns the same bits.  They are outside the magnitude contract (code -15 after a rescaled sharded solve).

"""    tsqr_products_hip(h, n, t, p=nothing; dJp=C_NULL) -> (grad, sums, Ap)

`grad = J'(rx + J p)` over all ranks (`p === nothing`: `J' rx`, src/enlsip_functions.jl:2690), `sums = (dot(rx,rx), dot(Jp,Jp),
dot(Jp,rx))` (:1561-1584, :2269), `Ap = C.A p` on the active rows (:2227; empty without `p`).  `dJp`: device pointer to `m_loc`
doubles that receive this rank's rows of `J p` (:2226), or C_NULL."""
function tsqr_products_hip(h::Handle, n::Integer, t::Integer, p::Union{Nothing,Vector{Float64}}=nothing;
                           dJp::Ptr{Float64}=Ptr{Float64}(C_NULL))
    grad = zeros(Float64, n); sums = zeros(Float64, 3)
    Ap = zeros(Float64, p === nothing ? 0 : t)
    pp = p === nothing ? Ptr{Float64}(C_NULL) : pointer(p)
    pa = isempty(Ap) ? Ptr{Float64}(C_NULL) : pointer(Ap)
    GC.@preserve p grad sums Ap check(h, ccall((:enlsip_gn_tsqr_products, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, pp, dJp, grad, sums, pa))
    return grad, sums, Ap
end

"""    tsqr_first_lagrange_hip(h, t, ε_rank; grad_fx=nothing, diag_scale=nothing) -> (λ, grad_res)

`first_lagrange_mult_estimate!` (src/enlsip_functions.jl:461-508) on the replicated `F_A` of the sharded solve; without `grad_fx`
the gradient `J' rx` is formed over the ranks (collective)."""
function tsqr_first_lagrange_hip(h::Handle, t::Integer, ε_rank::Float64; grad_fx::Union{Nothing,Vector{Float64}}=nothing,
                                 diag_scale::Union{Nothing,Vector{Float64}}=nothing)
    λ = zeros(Float64, t); gres = Ref{Float64}(0.0)
    pg = grad_fx === nothing ? Ptr{Float64}(C_NULL) : pointer(grad_fx)
    pd = diag_scale === nothing ? Ptr{Float64}(C_NULL) : pointer(diag_scale)
    GC.@preserve grad_fx diag_scale λ check(h, ccall((:enlsip_gn_tsqr_first_lagrange, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{Float64}), h.ptr, pg, pd, ε_rank, λ, gres))
    return λ, gres[]
end

"""    tsqr_second_lagrange_hip(h, t, p_gn, ε_rank; diag_scale=nothing) -> λ

`second_lagrange_mult_estimate!` (src/enlsip_functions.jl:514-537), collective: `J1'(rx + J p_gn)` is formed as
`(F_A.Q' (J'(rx + J p_gn)))[1:t]` from the shards' products."""
function tsqr_second_lagrange_hip(h::Handle, t::Integer, p_gn::Vector{Float64}, ε_rank::Float64;
                                  diag_scale::Union{Nothing,Vector{Float64}}=nothing)
    λ = zeros(Float64, t)
    pd = diag_scale === nothing ? Ptr{Float64}(C_NULL) : pointer(diag_scale)
    GC.@preserve p_gn diag_scale λ check(h, ccall((:enlsip_gn_tsqr_second_lagrange, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}), h.ptr, p_gn, pd, ε_rank, λ))
    return λ
end

"""    tsqr_newton_direction(h, Γ) -> (p, not_posdef)

`newton_search_direction` (src/enlsip_functions.jl:348-423) after its Hessian sums on the resident result of the handle's last
sharded solve: `Γ = r_mat - c_mat` (n x n).  Nothing is exchanged and no shard is read; ranks that pass the same `Γ` get the same
bits.  `not_posdef` is the reference's `error = true` (then `p` is zero)."""
function tsqr_newton_direction(h::Handle, Γ::Matrix{Float64})
    n = size(Γ, 1)
    size(Γ, 2) == n || throw(DimensionMismatch("Γ must be square"))
    p = zeros(Float64, n)
    bad = Ref{Int64}(0)
    GC.@preserve Γ p check(h, ccall((:enlsip_gn_tsqr_newton_direction, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}), h.ptr, Γ, n, p, bad))
    return p, bad[] != 0
end

"""    tsqr_products_local_hip!(h, dJ, ldj, drx, dp, dJp, dmsg, m_loc, n)

The local stage alone, for callers that move the messages themselves: device pointers in, the shard's message
(`tsqr_products_msg_len(n)` doubles) in `dmsg`.  `dp`, `dJp` may be C_NULL."""
function tsqr_products_local_hip!(h::Handle, dJ::Ptr{Float64}, ldj::Integer, drx::Ptr{Float64}, dp::Ptr{Float64},
                                  dJp::Ptr{Float64}, dmsg::Ptr{Float64}, m_loc::Integer, n::Integer)
    check(h, ccall((:enlsip_gn_tsqr_products_local_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h.ptr, m_loc, n, dJ, ldj, drx, dp, dJp, dmsg))
end

"""    tsqr_products_combine_hip(h, dmsgs, G, n) -> (grad, sums): the G gathered messages (device, rank-major) added in rank order"""
function tsqr_products_combine_hip(h::Handle, dmsgs::Ptr{Float64}, G::Integer, n::Integer)
    grad = zeros(Float64, n); sums = zeros(Float64, 3)
    GC.@preserve grad sums check(h, ccall((:enlsip_gn_tsqr_products_combine_dev, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, G, n, dmsgs, grad, sums))
    return grad, sums
end

"""    tsqr_products_msg_len(n): doubles per message — header (4), g (n), three sums, rounded up to 16-byte granules"""
tsqr_products_msg_len(n::Integer) = (4 + n + 3 + 1) & ~1

end # module

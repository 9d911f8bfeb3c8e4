# SLSMI355X.jl — the reference-side binding for libsls_mi355x.so (include/sls_mi355x.h).
#
# What a maintainer of aaltoKEPO/SystemLevelControl.jl adds to route `SLS_𝓗₂` through the MI355X engine:
# this file is pure `ccall` marshalling (no algorithm), ≈100 lines.  It replaces the body of
# src/synthesis.jl:11-32 (the @distributed loop over _SLS_𝓗₂) and nothing else; `Plant`, the masks and the
# returned `Φₓ,Φᵤ` (vectors of SparseMatrixCSC{Float64,Int}) are unchanged, so README.md:43-72 runs as is.
#
# NOT EXECUTED in the build container (no Julia there: SURVEY.md §0 F5).  The identical marshalling — same struct
# layouts, same argument order, index_base = 0 instead of 1 — is exercised by the Python ctypes binding
# (systemlevelcontrol.jl_amd/_capi.py) in tests/.
module SLSMI355X

using SparseArrays
export SLS_𝓗₂_mi355x, SLS_𝓗₂_mi355x_localized, sls_context, sls_close, default_ctx, sls_ridge!, objective_values, last_objective, update_plant!, update_weights!, weights, SLS_PLAN_WEIGHTS_UPDATABLE, track_changes!, execute_dirty!, residual, gradient, multipliers, SLS_PLAN_MULTIPLIERS, Controller, load!, reset!, step!, Rollout, set_plant!, set_weights!, run!, stats, Margin, margins, set_radius!, box_margins, worst_plant, Norms, l1, hinf, h2, covariance_pattern!, covariance

const LIB = get(ENV, "SLS_MI355X_LIB", "libsls_mi355x.so")

struct CscF64            # sls_csc_f64
    nrows::Int64; ncols::Int64
    colptr::Ptr{Int64}; rowval::Ptr{Int64}; nzval::Ptr{Float64}
end
struct CscBool           # sls_csc_bool  (Julia Bool is one byte: 0x00 / 0x01)
    nrows::Int64; ncols::Int64
    colptr::Ptr{Int64}; rowval::Ptr{Int64}; nzval::Ptr{UInt8}
end
struct Dims              # sls_dims
    Nx::Int64; Nu::Int64; Nz::Int64; Nw::Int64; T::Int64
    index_base::Int32; flags::UInt32
end
struct PlantPtrs         # sls_plant
    A::Ptr{CscF64}; B1::Ptr{CscF64}; B2::Ptr{CscF64}; C1::Ptr{CscF64}; D11::Ptr{CscF64}; D12::Ptr{CscF64}
end

csc(M::SparseMatrixCSC{Float64,Int}) = CscF64(size(M,1), size(M,2), pointer(M.colptr), pointer(M.rowval), pointer(M.nzval))
csc(M::SparseMatrixCSC{Bool,Int})    = CscBool(size(M,1), size(M,2), pointer(M.colptr), pointer(M.rowval),
                                               Ptr{UInt8}(pointer(M.nzval)))

"One context = the GPUs used, the analogue of the `julia -p N` worker pool (src/synthesis.jl:16)."
function sls_context(devices::Vector{<:Integer}=[0])
    devs = Int32.(devices)
    ctx = ccall((:sls_create, LIB), Ptr{Cvoid}, (Ptr{Int32}, Cint, UInt32), devs, length(devs), 0)
    ctx == C_NULL && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return ctx
end
sls_close(ctx) = ccall((:sls_destroy, LIB), Cvoid, (Ptr{Cvoid},), ctx)

# Lazily created process-wide context (what the one-line patch of src/synthesis.jl:11 in INTEGRATION.md calls): the devices
# come from ENV["SLS_MI355X_DEVICES"] ("0,1,2,3"; default "0"); it is destroyed at exit.
const _default_ctx = Ref{Ptr{Cvoid}}(C_NULL)
function default_ctx()
    if _default_ctx[] == C_NULL
        devs = parse.(Int, split(get(ENV, "SLS_MI355X_DEVICES", "0"), ","))
        _default_ctx[] = sls_context(devs)
        atexit() do
            _default_ctx[] != C_NULL && (sls_close(_default_ctx[]); _default_ctx[] = C_NULL)
        end
    end
    return _default_ctx[]
end

"""
    sls_ridge!(ctx, rₓ, rᵤ)

The diagonal quadratic instance of the reference's `L⁺` hook (src/synthesis.jl:21,52): every later solve on `ctx` adds
`Σₜ Σᵢ rₓ[i]·Φₓ[t][i,c]² + Σⱼ rᵤ[j]·Φᵤ[t][j,c]²` to each column's cost.  `sls_ridge!(ctx, Float64[], Float64[])` clears it.
"""
function sls_ridge!(ctx::Ptr{Cvoid}, rₓ::Vector{Float64}, rᵤ::Vector{Float64})
    rc = ccall((:sls_set_ridge, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
               ctx, length(rₓ), rₓ, length(rᵤ), rᵤ)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return nothing
end

"""
    J, total = objective_values(plan, d_values, nsub; packed=false)

`sls_plan_fetch_objective` on a resident plan (a `Ptr{Cvoid}` from `sls_h2_sf_plan`, `nsub` = its `n_subproblems`): the objective
value every subproblem achieved, evaluated on the device from the value array an execute wrote, and their sum — the
reference's `objective_value(problem)` (src/synthesis.jl:52) per column.  A coupled group's joint value sits on its first column.
"""
function objective_values(plan::Ptr{Cvoid}, d_values::Ptr{Cvoid}, nsub::Integer; packed::Bool=false)
    J = zeros(Float64, nsub);  total = Ref{Float64}(0.0)
    rc = ccall((:sls_plan_fetch_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ref{Float64}),
               plan, d_values, packed ? 1 : 0, J, total)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return J, total[]
end

"""
    n_rejected = update_plant!(plan, A, B2; stream=C_NULL, wait=true, nnzA=-1, nnzB2=-1)

`sls_plan_update_plant` on a resident plan (a `Ptr{Cvoid}` from `sls_h2_sf_plan`): new values of `A` and / or `B2` (a
`SparseMatrixCSC{Float64}`, a `Vector{Float64}` of `nzval`, or `nothing` = unchanged), host path; the next `sls_plan_execute`
solves the new plant without a rebuild.  UNCHECKED: a raw plan pointer carries no pattern, so the caller guarantees that a matrix
has the stored pattern the plan was built from and that a vector has exactly its `nnz` entries in that CSC order — a shorter array
makes the library read past its end.  Pass `nnzA` / `nnzB2` (the `nnz` of the plan's matrices) to have the lengths checked.  An entry that was exactly 0.0 when the
plan was built must stay 0.0 and every value must be finite, else the call errors (`SLS_EINVAL`) and the plan is untouched.  An
attached refinement is dropped.  With `wait = true` returns `sls_plan_update_result` (0 after a host-path update).
"""
function update_plant!(plan::Ptr{Cvoid}, A, B2; stream::Ptr{Cvoid}=C_NULL, wait::Bool=true, nnzA::Integer=-1, nnzB2::Integer=-1)
    nz(M::SparseMatrixCSC) = convert(Vector{Float64}, nonzeros(M))
    nz(v::AbstractVector) = convert(Vector{Float64}, v)
    nz(::Nothing) = nothing
    a, b = nz(A), nz(B2)
    (a !== nothing && nnzA >= 0 && length(a) != nnzA) && error("update_plant!: A has $(length(a)) values, the plan stores $nnzA")
    (b !== nothing && nnzB2 >= 0 && length(b) != nnzB2) && error("update_plant!: B2 has $(length(b)) values, the plan stores $nnzB2")
    GC.@preserve a b begin
        rc = ccall((:sls_plan_update_plant, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), plan, stream,
                   a === nothing ? Ptr{Float64}(C_NULL) : pointer(a), b === nothing ? Ptr{Float64}(C_NULL) : pointer(b), 0)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    wait || return 0
    n = Ref{Int64}(0)
    rc = ccall((:sls_plan_update_result, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), plan, n)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return n[]
end

"`sls_dims.flags` bit: build the plan so that `update_weights!` can give it new LQR weights (or it with the objective's flag)."
const SLS_PLAN_WEIGHTS_UPDATABLE = UInt32(2)

"""
    n_rejected = update_weights!(plan, c1, d12; Nx, Nu, stream=C_NULL, wait=true)

`sls_plan_update_weights` on a resident plan built with `SLS_PLAN_WEIGHTS_UPDATABLE` in `dims.flags` (a `Ptr{Cvoid}` from
`sls_h2_sf_plan`): new diagonals of `C1 = [diag(c1); 0]` and / or `D12 = [0; diag(d12)]` — a `Vector{Float64}` of the `Nx` / `Nu`
diagonal values, a `SparseMatrixCSC{Float64}` of that LQR shape (one stored entry per column, checked here; its `nzval` is the
diagonal) or `nothing` = unchanged — host path; the next `sls_plan_execute` solves the re-weighted problem without a rebuild.  A
raw plan pointer carries no sizes: pass the plant's `Nx` and `Nu`, the lengths are checked against them.  Every value must be
finite and keep the Hessian positive (0.0 needs a ridge term), else the call errors (`SLS_EINVAL`) and the plan is untouched.  An
attached refinement is dropped.  With `wait = true` returns `sls_plan_update_weights_result` (0 after a host-path update).
"""
function update_weights!(plan::Ptr{Cvoid}, c1, d12; Nx::Integer, Nu::Integer, stream::Ptr{Cvoid}=C_NULL, wait::Bool=true)
    function dg(M::SparseMatrixCSC, n, shift, name)
        (size(M) == (Nx + Nu, n) && nnz(M) == n && M.colptr == collect(1:n+1) && rowvals(M) == collect(1:n) .+ shift) ||
            error("update_weights!: $name must be $(Nx + Nu)×$n with one stored entry per column, column j on row $shift + j")
        return convert(Vector{Float64}, nonzeros(M))
    end
    dg(v::AbstractVector, n, shift, name) = length(v) == n ? convert(Vector{Float64}, v) :
        error("update_weights!: $name needs the $n diagonal values, got $(length(v))")
    dg(::Nothing, n, shift, name) = nothing
    c, d = dg(c1, Nx, 0, "C1"), dg(d12, Nu, Nx, "D12")
    (c === nothing && d === nothing) && error("update_weights!: give c1, d12 or both")
    GC.@preserve c d begin
        rc = ccall((:sls_plan_update_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), plan, stream,
                   c === nothing ? Ptr{Float64}(C_NULL) : pointer(c), d === nothing ? Ptr{Float64}(C_NULL) : pointer(d), 0)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    wait || return 0
    n = Ref{Int64}(0)
    rc = ccall((:sls_plan_update_weights_result, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), plan, n)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return n[]
end

"""
    c1, d12 = weights(plan; Nx, Nu)

`sls_plan_fetch_weights`: the diagonals of `C1` and `D12` the plan holds on the device now (waits for the plan's last update).
"""
function weights(plan::Ptr{Cvoid}; Nx::Integer, Nu::Integer)
    c, d = zeros(Float64, max(Nx, 1)), zeros(Float64, max(Nu, 1))
    rc = ccall((:sls_plan_fetch_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), plan, c, d)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return c[1:Nx], d[1:Nu]
end

"""
    r = residual(plan, d_values, nsub; packed=false)

`sls_plan_fetch_residual` on a resident plan (a `Ptr{Cvoid}` from `sls_h2_sf_plan`, `nsub` = its `n_subproblems`): the defect of
`Φₓ[1] = I`, `Φₓ[t+1] = A Φₓ[t] + B₂ Φᵤ[t]`, `0 = A Φₓ[T] + B₂ Φᵤ[T]` on ALL rows of the plant, per subproblem, evaluated on the
device from the value array `d_values` and the values of `A`, `B₂` the plan holds now (after `update_plant!`: the new ones, whether
or not the columns were solved again).  Returns a named tuple: `res_inf` (max |Δ| over the rows of s_x and the halo rows outside
it), `halo_inf` (the halo rows alone), `res_l1` (Σ|Δ|), each of length `nsub`, and `max_inf`, `e1_norm` = their maxima over the
subproblems — the latter is the 𝓔₁ norm robust SLS needs below 1.  Waits for the plan's last execute and last update.
"""
function residual(plan::Ptr{Cvoid}, d_values::Ptr{Cvoid}, nsub::Integer; packed::Bool=false)
    res_inf = zeros(Float64, nsub);  halo_inf = zeros(Float64, nsub);  res_l1 = zeros(Float64, nsub);  totals = zeros(Float64, 2)
    rc = ccall((:sls_plan_fetch_residual, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
               plan, d_values, packed ? 1 : 0, res_inf, halo_inf, res_l1, totals)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return (res_inf=res_inf, halo_inf=halo_inf, res_l1=res_l1, max_inf=totals[1], e1_norm=totals[2])
end

const SLS_PLAN_MULTIPLIERS = UInt32(4)      # sls_dims.flags: the plan keeps the multipliers every execute ends with

"""
    g = gradient(plan, d_values, nnzA, nnzB2; packed=false, column_weights=nothing, Nx=0, Nu=0)

`sls_plan_fetch_gradient` on a resident plan built with `SLS_PLAN_MULTIPLIERS` in `dims.flags`: the derivative of `Σ_j c_j J_j`
(`J_j` as `objective_values` reports it, `c_j = column_weights`, default 1) in every stored entry of `A` and `B₂`, in the `nzval`
order `update_plant!` takes, from the multipliers the last execute left and the values it wrote to `d_values`.  With `Nx`, `Nu`
given (plans that also have `SLS_PLAN_WEIGHTS_UPDATABLE`) also the derivatives in the diagonals of `C₁` and `D₁₂`.  Returns a
named tuple `gA`, `gB2`, `gc1`, `gd12` (the last two empty unless asked for) and `n_skipped`, the subproblems that contributed 0
because they are neither solved nor trivial.  Waits for the plan's last execute and last update.
"""
function gradient(plan::Ptr{Cvoid}, d_values::Ptr{Cvoid}, nnzA::Integer, nnzB2::Integer; packed::Bool=false,
                  column_weights::Union{Nothing,Vector{Float64}}=nothing, Nx::Integer=0, Nu::Integer=0)
    gA = zeros(Float64, max(nnzA, 1));  gB2 = zeros(Float64, max(nnzB2, 1))
    gc1 = zeros(Float64, max(Nx, 1));  gd12 = zeros(Float64, max(Nu, 1))
    nskip = Ref{Int64}(0)
    cw = column_weights === nothing ? Ptr{Float64}(C_NULL) : pointer(column_weights)
    rc = GC.@preserve column_weights ccall((:sls_plan_fetch_gradient, LIB), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
               plan, d_values, packed ? 1 : 0, cw, gA, gB2, Nx > 0 ? pointer(gc1) : Ptr{Float64}(C_NULL),
               Nu > 0 ? pointer(gd12) : Ptr{Float64}(C_NULL), nskip)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return (gA=gA[1:nnzA], gB2=gB2[1:nnzB2], gc1=gc1[1:Nx], gd12=gd12[1:Nu], n_skipped=nskip[])
end

"""
    μ = multipliers(plan, sub, T)

`sls_plan_fetch_multipliers`: the multiplier of subproblem `sub` (0-based, `col_status` order) as the last execute left it, a
`ñx × (T+1)` matrix — column `k+1` is block row `k` of the achievability constraints, rows in `sₓ` order.
"""
function multipliers(plan::Ptr{Cvoid}, sub::Integer, T::Integer)
    len = ccall((:sls_plan_fetch_multipliers, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), plan, sub, C_NULL, 0)
    len < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    mu = zeros(Float64, max(len, 1))
    rc = ccall((:sls_plan_fetch_multipliers, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), plan, sub, mu, len)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return reshape(mu[1:len], div(len, T + 1), T + 1)
end

"""
    track_changes!(plan, on=true)

`sls_plan_track_changes`: with tracking on, every later `update_plant!` also marks the subproblems touched by the entries it
actually changed; turning it on clears the marks.
"""
function track_changes!(plan::Ptr{Cvoid}, on::Bool=true)
    rc = ccall((:sls_plan_track_changes, LIB), Cint, (Ptr{Cvoid}, Cint), plan, on ? 1 : 0)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return nothing
end

"""
    n_solved = execute_dirty!(plan, d_values; packed=false, stream=C_NULL)

`sls_plan_execute_dirty`: re-solve only the marked subproblems into the device array `d_values`, then clear the marks on
`stream`.  Waits for `stream` once before the solve is enqueued; the solve itself is asynchronous like `sls_plan_execute`.
"""
function execute_dirty!(plan::Ptr{Cvoid}, d_values::Ptr{Cvoid}; packed::Bool=false, stream::Ptr{Cvoid}=C_NULL)
    n = Ref{Int64}(0)
    rc = ccall((:sls_plan_execute_dirty, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ref{Int64}), plan, stream, d_values,
               packed ? 1 : 0, n)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return n[]
end

"""
    c = Controller(ctx, Nx, Nu, [𝓢ₓ,𝓢ᵤ]; nscen=1, dev_slot=0)
    load!(c, d_values; stream=C_NULL);  reset!(c; stream=C_NULL);  step!(c, d_x, d_u; d_what=C_NULL, stream=C_NULL)

`sls_controller_*`: the stand-alone controller built from the masks alone — step `k` takes the measured state `d_x` (`[Nx][nscen]`
on the device) and writes `u_k = Σ_τ Φᵤ[τ] ŵ_{k+1−τ}` to `d_u` (`[Nu][nscen]`), with `ŵ_k = x_k − β_k` (to `d_what` when given) and
`β_{k+1} = Σ_τ Φₓ[τ+1] ŵ_{k+1−τ}` kept inside.  No plant is involved, so the state may come from any plant or from a measurement.
`load!` gathers Φ from the mask-order device array an execute filled and keeps β and the history; `reset!` clears them.  All three
enqueue on `stream` and return; the calls of one controller go to one stream.  `close(c)` frees it.  NOT EXECUTED in the build
container, like the rest of this file.
"""
mutable struct Controller
    handle::Ptr{Cvoid}
    Nx::Int; Nu::Int; nscen::Int
end
function Controller(ctx::Ptr{Cvoid}, Nx::Integer, Nu::Integer, 𝓢::AbstractVector; nscen::Integer=1, dev_slot::Integer=0)
    𝓢ₓ, 𝓢ᵤ = 𝓢
    Sx = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ₓ];  Su = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ᵤ]
    sx = [csc(S) for S in Sx];  su = [csc(S) for S in Su]
    dims = Ref(Dims(Nx, Nu, Nx + Nu, Nx, length(Sx), 1, UInt32(0)))       # only Nx, Nu, T, index_base are read
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Sx Su sx su begin
        rc = ccall((:sls_controller_plan, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Dims}, Ptr{CscBool}, Ptr{CscBool}, Int64, Ref{Ptr{Cvoid}}),
                   ctx, dev_slot, dims, sx, su, nscen, h)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return Controller(h[], Nx, Nu, nscen)
end
_ctl_check(rc) = (rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL))); nothing)
load!(c::Controller, d_values::Ptr{Cvoid}; stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_controller_load, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.handle, stream, d_values))
reset!(c::Controller; stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_controller_reset, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.handle, stream))
step!(c::Controller, d_x::Ptr{Cvoid}, d_u::Ptr{Cvoid}; d_what::Ptr{Cvoid}=C_NULL, stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_controller_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     c.handle, stream, d_x, d_u, d_what))
function Base.close(c::Controller)
    c.handle != C_NULL && (ccall((:sls_controller_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.handle); c.handle = C_NULL)
    return nothing
end

"""
    r = Rollout(ctx, P, [𝓢ₓ,𝓢ᵤ]; nscen=1, dev_slot=0)
    load!(r, d_values);  set_plant!(r, A_nzval, B2_nzval; per_scenario=false);  set_weights!(r, q, rr)
    reset!(r; d_x0=C_NULL);  run!(r, steps; d_w=C_NULL, d_x=C_NULL, d_u=C_NULL);  cost, peak_x, peak_u, x_now = stats(r)

`sls_rollout_*`: the closed-loop rollout of the Φ on the device against an ensemble of plants — scenario `s` has its own values of
`A` and `B₂` on `P`'s non-zero patterns (every scenario starts from `P`'s values), `B₁` and Φ are shared; the LQR cost
`Σ_k Σ_i (q_i x_k[i])² + Σ_j (r_j u_k[j])²` and the peaks of `|x|`, `|u|` are accumulated on the device and memory does not depend on
the number of steps.  `set_plant!` takes `nzval` vectors in `P`'s own CSC order (`nothing` keeps; `per_scenario=true`: a
`nscen × nnz` matrix, scenario innermost in memory) and is not validated; `set_weights!` takes `q` (`Nx`) and `rr` (`Nu`).  `reset!`,
`run!` and `load!` enqueue on `stream` and return (`d_w`, `d_x`, `d_u`, `d_x0`: device pointers, `[steps][N·][nscen]`); `stats` waits
and returns host vectors of length `nscen` and the current state (`nscen × Nx`).  `close(r)` frees it.  NOT EXECUTED in the build
container, like the rest of this file.
"""
mutable struct Rollout
    handle::Ptr{Cvoid}
    Nx::Int; Nu::Int; nscen::Int
end
function Rollout(ctx::Ptr{Cvoid}, P, 𝓢::AbstractVector; nscen::Integer=1, dev_slot::Integer=0)
    𝓢ₓ, 𝓢ᵤ = 𝓢
    f64(M) = SparseMatrixCSC{Float64,Int}(M)
    A, B1, B2 = f64(P.A), f64(P.B₁), f64(P.B₂)
    Sx = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ₓ];  Su = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ᵤ]
    mats = [csc(A), csc(B1), csc(B2)]
    sx = [csc(S) for S in Sx];  su = [csc(S) for S in Su]
    dims = Ref(Dims(P.Nx, P.Nu, P.Nz, P.Nw, length(Sx), 1, UInt32(0)))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A B1 B2 mats Sx Su sx su begin
        pm = pointer(mats)
        plant = Ref(PlantPtrs(pm, pm + sizeof(CscF64), pm + 2sizeof(CscF64), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL)))
        rc = ccall((:sls_rollout_plan, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Dims}, Ref{PlantPtrs}, Ptr{CscBool}, Ptr{CscBool}, Int64, Ref{Ptr{Cvoid}}),
                   ctx, dev_slot, dims, plant, sx, su, nscen, h)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return Rollout(h[], P.Nx, P.Nu, nscen)
end
load!(r::Rollout, d_values::Ptr{Cvoid}; stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_rollout_load, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), r.handle, stream, d_values))
_nzptr(v) = v === nothing ? Ptr{Float64}(C_NULL) : pointer(v)
function set_plant!(r::Rollout, A_nzval::Union{Nothing,Array{Float64}}, B2_nzval::Union{Nothing,Array{Float64}}; per_scenario::Bool=false,
                    stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve A_nzval B2_nzval begin                                 # host arrays: the call returns after they have been copied
        _ctl_check(ccall((:sls_rollout_set_plant, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Cint),
                         r.handle, stream, _nzptr(A_nzval), _nzptr(B2_nzval), 0, per_scenario ? 1 : 0))
    end
end
function set_weights!(r::Rollout, q::Union{Nothing,Vector{Float64}}, rr::Union{Nothing,Vector{Float64}}; stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve q rr begin
        _ctl_check(ccall((:sls_rollout_set_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                         r.handle, stream, _nzptr(q), _nzptr(rr), 0))
    end
end
reset!(r::Rollout; d_x0::Ptr{Cvoid}=C_NULL, stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_rollout_reset, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), r.handle, stream, d_x0))
run!(r::Rollout, steps::Integer; d_w::Ptr{Cvoid}=C_NULL, d_x::Ptr{Cvoid}=C_NULL, d_u::Ptr{Cvoid}=C_NULL, stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_rollout_run, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                     r.handle, stream, d_w, steps, d_x, d_u))
function stats(r::Rollout; stream::Ptr{Cvoid}=C_NULL)
    cost, px, pu = zeros(r.nscen), zeros(r.nscen), zeros(r.nscen)
    x = zeros(r.nscen, r.Nx)                                            # column-major (nscen, Nx) = the library's [Nx][nscen]
    _ctl_check(ccall((:sls_rollout_fetch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     r.handle, stream, x, cost, px, pu))
    return cost, px, pu, x
end
function Base.close(r::Rollout)
    r.handle != C_NULL && (ccall((:sls_rollout_destroy, LIB), Cvoid, (Ptr{Cvoid},), r.handle); r.handle = C_NULL)
    return nothing
end

"""
    m = Margin(ctx, P, [𝓢ₓ,𝓢ᵤ]; nscen=1, dev_slot=0)
    load!(m, d_values);  set_plant!(m, A_nzval, B2_nzval; per_scenario=false);  row_l1, col_l1, l1, e1 = margins(m)

`sls_margin_*`: robust-stability margins of the Φ on the device for an ensemble of plants — scenario `s` has its own values of `A`
and `B₂` on `P`'s non-zero patterns (every scenario starts from `P`'s values).  `D⁽ˢ⁾[τ] = Φₓ[τ+1] − A⁽ˢ⁾Φₓ[τ] − B₂⁽ˢ⁾Φᵤ[τ]` (0-based
slices, `Φₓ[0] := I`); `row_l1` and `col_l1` (`nscen × Nx`) are its absolute row and column sums, `l1[s] = ‖D⁽ˢ⁾‖_𝓛₁` and
`e1[s] = ‖D⁽ˢ⁾‖_𝓔₁` their maxima: below 1 the loop on plant `s` is internally stable, and `‖ŵ‖∞ ≤ ‖w̃‖∞/(1 − l1[s])`.  `set_plant!`
is the rollout's; `margins` waits.  `close(m)` frees it.  NOT EXECUTED in the build container, like the rest of this file.
"""
mutable struct Margin
    handle::Ptr{Cvoid}
    Nx::Int; Nu::Int; nscen::Int
    nnzA::Int; nnzB2::Int
end
function Margin(ctx::Ptr{Cvoid}, P, 𝓢::AbstractVector; nscen::Integer=1, dev_slot::Integer=0)
    𝓢ₓ, 𝓢ᵤ = 𝓢
    f64(M) = SparseMatrixCSC{Float64,Int}(M)
    A, B1, B2 = f64(P.A), f64(P.B₁), f64(P.B₂)
    Sx = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ₓ];  Su = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ᵤ]
    mats = [csc(A), csc(B1), csc(B2)]
    sx = [csc(S) for S in Sx];  su = [csc(S) for S in Su]
    dims = Ref(Dims(P.Nx, P.Nu, P.Nz, P.Nw, length(Sx), 1, UInt32(0)))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A B1 B2 mats Sx Su sx su begin
        pm = pointer(mats)
        plant = Ref(PlantPtrs(pm, pm + sizeof(CscF64), pm + 2sizeof(CscF64), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL)))
        rc = ccall((:sls_margin_plan, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Dims}, Ref{PlantPtrs}, Ptr{CscBool}, Ptr{CscBool}, Int64, Ref{Ptr{Cvoid}}),
                   ctx, dev_slot, dims, plant, sx, su, nscen, h)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return Margin(h[], P.Nx, P.Nu, nscen, nnz(A), nnz(B2))
end
load!(m::Margin, d_values::Ptr{Cvoid}; stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_margin_load, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), m.handle, stream, d_values))
function set_plant!(m::Margin, A_nzval::Union{Nothing,Array{Float64}}, B2_nzval::Union{Nothing,Array{Float64}}; per_scenario::Bool=false,
                    stream::Ptr{Cvoid}=C_NULL)
    GC.@preserve A_nzval B2_nzval begin                                 # host arrays: the call returns after they have been copied
        _ctl_check(ccall((:sls_margin_set_plant, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint, Cint),
                         m.handle, stream, _nzptr(A_nzval), _nzptr(B2_nzval), 0, per_scenario ? 1 : 0))
    end
end
function margins(m::Margin; stream::Ptr{Cvoid}=C_NULL)
    row, col = zeros(m.nscen, m.Nx), zeros(m.nscen, m.Nx)               # column-major (nscen, Nx) = the library's [Nx][nscen]
    tot = zeros(m.nscen, 2)
    _ctl_check(ccall((:sls_margin_fetch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     m.handle, stream, row, col, tot))
    return row, col, tot[:, 1], tot[:, 2]
end
"""
    set_radius!(m, A_rad, B2_rad; per_scenario=false);  row_wc, vertex, exact, l1_wc = box_margins(m);  A_nzval, B2_nzval = worst_plant(m)

The worst case over a box of plants (`sls_margin_set_radius`, `sls_margin_box_*`): every stored `A[i,k]`, `B₂[i,m]` is known to ± a
radius (host arrays in `nzval` order, `nothing` = zeros, `nnz` values or `nscen × nnz`) round the centre `set_plant!` set.  `row_wc`
(`nscen × Nx`) is the largest absolute row sum of `D` over the box, `vertex` the sign pattern that attains it (bit `b` set: centre +
radius of the row's `b`-th active coefficient; `-1`: a row with more than 10 active coefficients, which reports the triangle bound and
has `exact` false), `l1_wc[s]` the worst `‖D‖_𝓛₁`: below 1 the loop is stable on every plant of the box.  `worst_plant` returns the
plant (`nscen × nnz` each) that takes every row's vertex, fit for `set_plant!(…; per_scenario=true)` here and on a `Rollout`.
`set_radius!` is a setup call (allocates, waits); the others wait for `stream`.  NOT EXECUTED in the build container.
"""
function set_radius!(m::Margin, A_rad::Union{Nothing,Array{Float64}}, B2_rad::Union{Nothing,Array{Float64}}; per_scenario::Bool=false)
    GC.@preserve A_rad B2_rad begin
        _ctl_check(ccall((:sls_margin_set_radius, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint),
                         m.handle, _nzptr(A_rad), _nzptr(B2_rad), per_scenario ? 1 : 0))
    end
end
function box_margins(m::Margin; stream::Ptr{Cvoid}=C_NULL)
    row, ver = zeros(m.nscen, m.Nx), zeros(Int64, m.nscen, m.Nx)        # column-major (nscen, Nx) = the library's [Nx][nscen]
    ex, tot = zeros(UInt8, m.Nx), zeros(m.nscen)
    _ctl_check(ccall((:sls_margin_box_fetch, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}),
                     m.handle, stream, row, ver, ex, tot))
    return row, ver, ex .!= 0, tot
end
function worst_plant(m::Margin; stream::Ptr{Cvoid}=C_NULL)
    A, B2 = zeros(m.nscen, m.nnzA), zeros(m.nscen, m.nnzB2)             # column-major (nscen, nnz) = the library's [nnz][nscen]
    _ctl_check(ccall((:sls_margin_box_worst_plant, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), m.handle, stream, A, B2))
    return A, B2
end
function Base.close(m::Margin)
    m.handle != C_NULL && (ccall((:sls_margin_destroy, LIB), Cvoid, (Ptr{Cvoid},), m.handle); m.handle = C_NULL)
    return nothing
end

"""
    n = Norms(ctx, Nx, Nu, [𝓢ₓ,𝓢ᵤ]; cz=nothing, b=nothing, max_freq=64, dev_slot=0)
    load!(n, d_values; stream=C_NULL);  row_l1, col_l1, totals = l1(n);  sigma, peak, argpeak = hinf(n, ω; iters=32)

`sls_norms_*`: closed-loop 𝓛₁ and 𝓗∞ norms of the Φ on the device, built from the masks alone.  Rows are the `Nx` state rows
followed by the `Nu` input rows; `G[t] = diag(cz)·[Φₓ[t]; Φᵤ[t]]·diag(b)` for every `t` (Φₓ[1] = I included), `cz` of length `Nx+Nu`
and `b` of length `Nx`, `nothing` = ones (diagonal weights only).  `l1` returns the absolute row and column sums of `G` and
`totals = (𝓛₁ norm, 𝓔₁ norm)`; `hinf` returns, per angle of `ω` (radians per sample, at most `max_freq` of them), a power-iteration
lower bound of `σ_max(G(ω))`, their maximum and the 1-based index of the first angle that attains it.  The peak bounds the 𝓗∞ norm
from below on the grid `ω` only: refining the grid is the caller's business.  Both wait for `stream`.  `close(n)` frees it.  NOT
EXECUTED in the build container, like the rest of this file.
"""
mutable struct Norms
    handle::Ptr{Cvoid}
    Nx::Int; Nu::Int; max_freq::Int
    npairs::Int                                                          # of the covariance pattern in place (0 = none)
end
function Norms(ctx::Ptr{Cvoid}, Nx::Integer, Nu::Integer, 𝓢::AbstractVector; cz::Union{Nothing,Vector{Float64}}=nothing,
               b::Union{Nothing,Vector{Float64}}=nothing, max_freq::Integer=64, dev_slot::Integer=0)
    𝓢ₓ, 𝓢ᵤ = 𝓢
    Sx = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ₓ];  Su = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ᵤ]
    sx = [csc(S) for S in Sx];  su = [csc(S) for S in Su]
    cz === nothing || length(cz) == Nx + Nu || error("cz must have Nx + Nu entries")
    b === nothing || length(b) == Nx || error("b must have Nx entries")
    dims = Ref(Dims(Nx, Nu, Nx + Nu, Nx, length(Sx), 1, UInt32(0)))       # only Nx, Nu, T, index_base are read
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Sx Su sx su cz b begin
        rc = ccall((:sls_norms_plan, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ref{Dims}, Ptr{CscBool}, Ptr{CscBool}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Ptr{Cvoid}}),
                   ctx, dev_slot, dims, sx, su, cz === nothing ? C_NULL : pointer(cz), b === nothing ? C_NULL : pointer(b), max_freq, h)
    end
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return Norms(h[], Nx, Nu, max_freq, 0)
end
load!(n::Norms, d_values::Ptr{Cvoid}; stream::Ptr{Cvoid}=C_NULL) =
    _ctl_check(ccall((:sls_norms_load, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), n.handle, stream, d_values))
function l1(n::Norms; stream::Ptr{Cvoid}=C_NULL)
    row = zeros(Float64, n.Nx + n.Nu);  col = zeros(Float64, n.Nx);  totals = zeros(Float64, 2)
    _ctl_check(ccall((:sls_norms_fetch_l1, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     n.handle, stream, row, col, totals))
    return row, col, totals
end
function hinf(n::Norms, ω::AbstractVector{<:Real}; iters::Integer=32, stream::Ptr{Cvoid}=C_NULL)
    om = Vector{Float64}(ω);  sigma = zeros(Float64, length(om));  peak = zeros(Float64, 2)
    _ctl_check(ccall((:sls_norms_fetch_hinf, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                     n.handle, stream, om, length(om), iters, sigma, peak))
    return sigma, peak[1], Int(peak[2]) + 1
end
"""
    row_h2, col_h2, totals = h2(n);   covariance_pattern!(n, pairs_i, pairs_j);   cov = covariance(n)

`sls_norms_fetch_h2`, `sls_norms_cov_pattern`, `sls_norms_fetch_cov`.  `row_h2[i] = Σₜ Σⱼ G[t][i,j]²` is the variance of `zᵢ` under
unit white `w` (its square root the RMS of that state or actuator), `col_h2[j]` the share of disturbance `j`, `totals = (Σ row_h2,
max row_h2)`.  `covariance_pattern!` sets the entries `(pairs_i[p], pairs_j[p])` (1-based rows: states, then inputs) of
`Σ = Σₜ G[t]·G[t]ᵀ` that `covariance` evaluates — any order, duplicates and `i == j` allowed, empty lists clear the pattern; it
uploads and allocates, so call it once per pattern.  `h2` and `covariance` wait for `stream`.  NOT EXECUTED in the build
container, like the rest of this file.
"""
function h2(n::Norms; stream::Ptr{Cvoid}=C_NULL)
    row = zeros(Float64, n.Nx + n.Nu);  col = zeros(Float64, n.Nx);  totals = zeros(Float64, 2)
    _ctl_check(ccall((:sls_norms_fetch_h2, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     n.handle, stream, row, col, totals))
    return row, col, totals
end
function covariance_pattern!(n::Norms, pairs_i::AbstractVector{<:Integer}, pairs_j::AbstractVector{<:Integer})
    length(pairs_i) == length(pairs_j) || error("pairs_i and pairs_j must have one length")
    ip = Vector{Int64}(pairs_i);  jp = Vector{Int64}(pairs_j)
    _ctl_check(ccall((:sls_norms_cov_pattern, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}), n.handle, length(ip), ip, jp))
    n.npairs = length(ip)
    return n
end
function covariance(n::Norms; stream::Ptr{Cvoid}=C_NULL)
    cov = zeros(Float64, n.npairs)
    _ctl_check(ccall((:sls_norms_fetch_cov, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), n.handle, stream, cov))
    return cov
end
function Base.close(n::Norms)
    n.handle != C_NULL && (ccall((:sls_norms_destroy, LIB), Cvoid, (Ptr{Cvoid},), n.handle); n.handle = C_NULL)
    return nothing
end

"""
    J, total = last_objective(ctx, nsub)

`sls_ctx_last_objective`: the values of the last one-shot solve on `ctx` that ran with `return_objective = true`
(`sls_ctx_want_objective`), in the order of `status`.
"""
function last_objective(ctx::Ptr{Cvoid}, nsub::Integer)
    J = zeros(Float64, nsub);  total = Ref{Float64}(0.0)
    rc = ccall((:sls_ctx_last_objective, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Float64}), ctx, J, nsub, total)
    rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
    return J, total[]
end

"""
    Φₓ,Φᵤ = SLS_𝓗₂_mi355x(ctx, P, [𝓢ₓ,𝓢ᵤ]; 𝓘=nothing, objective=:h2, return_objective=false)

`return_objective = true` returns `Φₓ, Φᵤ, J, total` instead: `J[k]` is the objective value of subproblem k (the order of
`status`), evaluated on the device before the download, `total` their sum (the squared 𝓗₂ norm of the closed loop).

`objective = :sum_of_norms` minimises, per column, `Σₜ‖[C̃₁ D̃₁₂]Φ̃[t]B̃₁‖₂` instead (the column-separable bound of the 𝓗∞ norm;
`SLS_SOLVE_SUM_OF_NORMS` — not in the reference, which has no 𝓗∞ synthesis).

Drop-in for `SLS_𝓗₂(P, 𝓢; 𝓘)` (src/synthesis.jl:11).  `P` is any state-feedback plant exposing the reference's
fields (`A,B₁,B₂,C₁,D₁₁,D₁₂,Nx,Nu,Nz,Nw`); anything else returns `nothing`, like the reference (src/synthesis.jl:13,30).
"""
SLS_𝓗₂_mi355x(P, 𝓢::AbstractVector; kw...) = SLS_𝓗₂_mi355x(default_ctx(), P, 𝓢; kw...)
function SLS_𝓗₂_mi355x(ctx::Ptr{Cvoid}, P, 𝓢::AbstractVector; 𝓘=nothing, status::Union{Nothing,Vector{Int32}}=nothing,
                        objective::Symbol=:h2, return_objective::Bool=false)
    hasproperty(P, :C₂) && size(P.D₂₁, 1) == 0 || return nothing          # StateFeedback only
    𝓢ₓ, 𝓢ᵤ = 𝓢
    T = length(𝓢ₓ)
    f64(M) = SparseMatrixCSC{Float64,Int}(M)
    A, B1, B2, C1, D11, D12 = f64(P.A), f64(P.B₁), f64(P.B₂), f64(P.C₁), f64(P.D₁₁), f64(P.D₁₂)
    Sx = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ₓ];  Su = [SparseMatrixCSC{Bool,Int}(S) for S in 𝓢ᵤ]
    mats = [csc(A), csc(B1), csc(B2), csc(C1), csc(D11), csc(D12)]
    sx = [csc(S) for S in Sx];  su = [csc(S) for S in Su]
    flags = objective === :sum_of_norms ? UInt32(1) : UInt32(0)               # SLS_SOLVE_SUM_OF_NORMS
    dims = Ref(Dims(P.Nx, P.Nu, P.Nz, P.Nw, T, 1, flags))                  # index_base = 1: Julia's own arrays, no copy
    if 𝓘 === nothing
        ng, gptr, gcols = 0, Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL);  nsub = P.Nx
        keep = nothing
    else
        gp = Int64[0; cumsum(length.(𝓘))];  gc = Int64.(reduce(vcat, 𝓘))
        ng, gptr, gcols, nsub, keep = length(𝓘), pointer(gp), pointer(gc), length(gc), (gp, gc)
    end
    vx = [zeros(Float64, nnz(S)) for S in Sx];  vu = [zeros(Float64, nnz(S)) for S in Su]
    px = [pointer(v) for v in vx];  pu = [pointer(v) for v in vu]
    st = status === nothing ? zeros(Int32, nsub) : resize!(status, nsub)
    GC.@preserve A B1 B2 C1 D11 D12 Sx Su mats sx su vx vu px pu st keep begin
        pm = pointer(mats)
        plant = Ref(PlantPtrs(pm, pm + sizeof(CscF64), pm + 2sizeof(CscF64), pm + 3sizeof(CscF64),
                              pm + 4sizeof(CscF64), pm + 5sizeof(CscF64)))
        return_objective && ccall((:sls_ctx_want_objective, LIB), Cint, (Ptr{Cvoid}, Cint), ctx, 1)
        rc = ccall((:sls_h2_sf_solve, LIB), Cint,
                   (Ptr{Cvoid}, Ref{Dims}, Ref{PlantPtrs}, Ptr{CscBool}, Ptr{CscBool}, Int64, Ptr{Int64}, Ptr{Int64},
                    Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Int32}, Ptr{Cvoid}),
                   ctx, dims, plant, sx, su, ng, gptr, gcols, px, pu, st, C_NULL)
        return_objective && ccall((:sls_ctx_want_objective, LIB), Cint, (Ptr{Cvoid}, Cint), ctx, 0)
        rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
        rc > 0 && @warn "SLS_𝓗₂: $rc column(s) not solved to tolerance (see `status`; the reference never checks Ipopt's status)"
    end
    # values arrive in the masks' own CSC order ⇒ the pattern is the mask's, bit for bit; dropzeros! reproduces what
    # the reference's sparse `+` accumulation does to numerical zeros (src/synthesis.jl:65-67)
    Φₓ = [dropzeros!(SparseMatrixCSC(P.Nx, P.Nx, copy(S.colptr), copy(S.rowval), v)) for (S, v) in zip(Sx, vx)]
    Φᵤ = [dropzeros!(SparseMatrixCSC(P.Nu, P.Nx, copy(S.colptr), copy(S.rowval), v)) for (S, v) in zip(Su, vu)]
    return_objective && return (Φₓ, Φᵤ, last_objective(ctx, nsub)...)
    return Φₓ, Φᵤ
end

"""
    Φₓ,Φᵤ = SLS_𝓗₂_mi355x_localized(ctx, P, d, α, T)

The same solve for the README's own masks (README.md:52-54) given as `(d, α, T)`: `sls_h2_sf_solve_localized` builds index sets,
mask slices and destinations on the device — no mask array crosses PCIe.  The patterns of the returned matrices are the README
recipe's, computed here in Julia only to wrap the value arrays (a caller that keeps Φ on the device does not need them).
Default plant weights and default groups only (the library says so otherwise).
"""
function SLS_𝓗₂_mi355x_localized(ctx::Ptr{Cvoid}, P, d::Integer, α::Real, T::Integer)
    hasproperty(P, :C₂) && size(P.D₂₁, 1) == 0 || return nothing
    f64(M) = SparseMatrixCSC{Float64,Int}(M)
    A, B1, B2 = f64(P.A), f64(P.B₁), f64(P.B₂)
    Ab, Bb = (A .≠ 0), (SparseMatrixCSC(B2') .≠ 0)
    Sx = [SparseMatrixCSC{Bool,Int}((Ab^min(d, floor(Int, α * (t - 1)))) .≠ 0) for t in 1:T]
    Su = [SparseMatrixCSC{Bool,Int}((Bb * Ab^min(d + 1, floor(Int, α * (t - 1)))) .≠ 0) for t in 1:T]
    mats = [csc(A), csc(B1), csc(B2)]
    dims = Ref(Dims(P.Nx, P.Nu, P.Nz, P.Nw, T, 1, UInt32(0)))
    vx = [zeros(Float64, nnz(S)) for S in Sx];  vu = [zeros(Float64, nnz(S)) for S in Su]
    px = [pointer(v) for v in vx];  pu = [pointer(v) for v in vu]
    st = zeros(Int32, P.Nx)
    GC.@preserve A B1 B2 mats vx vu px pu st begin
        pm = pointer(mats)
        plant = Ref(PlantPtrs(pm, pm + sizeof(CscF64), pm + 2sizeof(CscF64), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL), Ptr{CscF64}(C_NULL)))
        rc = ccall((:sls_h2_sf_solve_localized, LIB), Cint,
                   (Ptr{Cvoid}, Ref{Dims}, Ref{PlantPtrs}, Int64, Cdouble, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Int32}, Ptr{Cvoid}),
                   ctx, dims, plant, d, α, px, pu, st, C_NULL)
        rc < 0 && error(unsafe_string(ccall((:sls_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx)))
        rc > 0 && @warn "SLS_𝓗₂: $rc column(s) not solved to tolerance"
    end
    Φₓ = [dropzeros!(SparseMatrixCSC(P.Nx, P.Nx, copy(S.colptr), copy(S.rowval), v)) for (S, v) in zip(Sx, vx)]
    Φᵤ = [dropzeros!(SparseMatrixCSC(P.Nu, P.Nx, copy(S.colptr), copy(S.rowval), v)) for (S, v) in zip(Su, vu)]
    return Φₓ, Φᵤ
end

end # module

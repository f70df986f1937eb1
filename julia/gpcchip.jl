# gpcchip.jl -- the reference-side binding of libgpcc_hip.so (include/gpcc_hip.h) a GPCC.jl maintainer would add as
# src/gpcchip.jl and `include` from src/GPCC.jl.  INTEGRATION.md section 1 explains it and shows the two edits inside GPCC.jl.
# NEVER EXECUTED: the build image has no Julia toolchain (SURVEY.md section 8(c)); syntax-reviewed only.  The same C ABI is
# exercised end to end by the Python ctypes host (gpcc.jl_amd/) and from plain C (tests/abi/abi_smoke.c).
# Thin ccall layer over include/gpcc_hip.h.  Host logic (parameter transforms, Nelder–Mead,
# restarts, printing) stays in gpccfixdelay_marginaliseb.jl untouched.
module GPCCHip

using Random, Statistics, LinearAlgebra, Distributions, MiscUtil    # all already dependencies of GPCC.jl

const LIB = get(ENV, "GPCC_HIP_LIB", "libgpcc_hip.so")

# Several Julia tasks / threads of ONE process, each with its own handle, each calling objective(α, ρ) (the pmap shape inside a process):
# the HIP runtime spreads a process's streams over 4 hardware queues by default, so at most 4 launches run side by side.  8 queues:
# 14 700 - 18 200 instead of 10 300 - 13 700 evaluations/s in total for 8 callers at N = 1024 (profiles/r05/concurrent_callers_round5b.log).
# Must be in the environment before the first HIP call of the process, i.e. before the library is used.
haskey(ENV, "GPU_MAX_HW_QUEUES") || (ENV["GPU_MAX_HW_QUEUES"] = "8")

# kernel function identity -> id (src/util.jl:15-52); any other callable stays on the Julia path
# (`include`d from src/GPCC.jl, this module's parent IS GPCC -- `Main.GPCC` would only exist after `using GPCC` in Main)
const _G = parentmodule(@__MODULE__)
kernelid(k) = k === _G.OU ? 0 : k === _G.rbf ? 1 :
              k === _G.matern32 ? 2 : k === _G.matern52 ? 3 : -1

lasterror(h) = unsafe_string(ccall((:gpcc_last_error, LIB), Cstring, (Ptr{Cvoid},), h))

mutable struct Handle
    ptr::Ptr{Cvoid}
    L::Int
end

"Replaces the precompute at gpccfixdelay_marginaliseb.jl:85-98 (marginalise_b=false: gpccfixdelay.jl:85-96)."
function create(tarray, yarray, stdarray; kernel, marginalise_b = true, device = 0)
    id = kernelid(kernel)
    id < 0 && return nothing                      # caller keeps the pure-Julia objective
    L  = length(tarray)
    Nl = Cint.(length.(tarray))
    t, y, s = reduce(vcat, tarray), reduce(vcat, yarray), reduce(vcat, stdarray)   # band order, user order
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:gpcc_create, LIB), Cint,
               (Ref{Ptr{Cvoid}}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint),
               ref, L, Nl, Float64.(t), Float64.(y), Float64.(s), id, marginalise_b ? 1 : 0, 0, device)
    rc == 0 || error("gpcc_create: " * lasterror(C_NULL))
    h = Handle(ref[], L)
    finalizer(x -> ccall((:gpcc_destroy, LIB), Cint, (Ptr{Cvoid},), x.ptr), h)
    return h
end

"objective for M triples.  delays, alpha: L×M Matrix{Float64} (column-major L×M == row-major M×L of the ABI)."
function loglik_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_loglik_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, info)
    rc == 0 || error("gpcc_loglik_batch: " * lasterror(h.ptr))
    return ll, info
end

"objective for M triples in LINEAR time (gpcc_loglik_markov_batch: a Kalman filter over the observations merged by shifted time; OU,
matern32, matern52 -- the same value as loglik_batch to rounding, DESIGN 4.15).  info as loglik_batch; a positive value is the merged
position of the first predictive variance that is not positive.  Errors for rbf and for marginalise_b with more than 4 bands."
function loglik_markov_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_loglik_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, info)
    rc == 0 || error("gpcc_loglik_markov_batch: " * lasterror(h.ptr))
    return ll, info
end

"predict_batch in LINEAR time (gpcc_predict_markov_batch: two Kalman filters and a combine per row, DESIGN 4.16; OU, matern32, matern52):
(mu T×M, var T×M, ll[M], info[M]) and, with weights, (mix_mu[T], mix_var[T]) -- what predict_batch returns, to rounding.  ttest: a
vector of L vectors, any order.  info = N + j: the combine of test point j failed (that column NaN)."
function predict_markov_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                              ttest::Vector{Vector{Float64}}; weights::Union{Nothing,Vector{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    Nt, tt = Cint.(length.(ttest)), reduce(vcat, ttest)
    T = length(tt)
    mu, var = Matrix{Float64}(undef, T, M), Matrix{Float64}(undef, T, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mm, mv = Vector{Float64}(undef, T), Vector{Float64}(undef, T)
    w = weights === nothing ? C_NULL : pointer(weights)
    GC.@preserve weights begin
        rc = ccall((:gpcc_predict_markov_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                   h.ptr, M, delays, alpha, rho, Nt, tt, w, mu, var, weights === nothing ? C_NULL : pointer(mm),
                   weights === nothing ? C_NULL : pointer(mv), ll, info)
    end
    rc == 0 || error("gpcc_predict_markov_batch: " * lasterror(h.ptr))
    return mu, var, ll, info, (weights === nothing ? nothing : (mm, mv))
end

"heldout_loglik_batch in LINEAR time (gpcc_heldout_loglik_markov_batch: loglik(training ∪ test) − loglik(training), two filters per
row): (heldout[M], ll[M], info[M], mix or nothing).  info = N + j: the predictive variance of test point j was not positive and finite."
function heldout_loglik_markov_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                     ttest::Vector{Vector{Float64}}, ytest::Vector{Vector{Float64}}, sigmatest::Vector{Vector{Float64}};
                                     weights::Union{Nothing,Vector{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == length(ytest) == length(sigmatest) == h.L
    @assert length.(ttest) == length.(ytest) == length.(sigmatest)
    Nt, tt, yt, st = Cint.(length.(ttest)), reduce(vcat, ttest), reduce(vcat, ytest), reduce(vcat, sigmatest)
    held, ll, info = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mix = Vector{Float64}(undef, 1)
    GC.@preserve weights begin
        rc = ccall((:gpcc_heldout_loglik_markov_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                   h.ptr, M, delays, alpha, rho, Nt, tt, yt, st, weights === nothing ? C_NULL : pointer(weights), held,
                   weights === nothing ? C_NULL : pointer(mix), ll, info)
    end
    rc == 0 || error("gpcc_heldout_loglik_markov_batch: " * lasterror(h.ptr))
    return held, ll, info, (weights === nothing ? nothing : mix[1])
end

"Exact leave-one-out predictive scores at M rows (gpcc_loo_batch; linear = true: gpcc_loo_markov_batch, OU / matern32 / matern52 in
linear time): for every training point i, in the order the light curves were handed over, the mean, variance and log-density of y_i
given every other observation, under the model of objective(alpha, rho) (no JITTER) -> (mu N×M, var N×M, lp N×M, loo[M], ll[M], info[M],
mix) with mix = nothing, or with weights (mix_lp[N], mix_loo): mix_lp_i = -log sum_m p_m exp(-lp_mi), the exact LOO log-density of the
delay mixture.  info = N + i: point i is the first whose variance is not positive and finite (the column is NaN)."
function loo_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64};
                   weights::Union{Nothing,Vector{Float64}} = nothing, linear::Bool = false)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    N = Int(ccall((:gpcc_get_option, LIB), Clong, (Ptr{Cvoid}, Cstring), h.ptr, "N"))
    mu, var, lp = Matrix{Float64}(undef, N, M), Matrix{Float64}(undef, N, M), Matrix{Float64}(undef, N, M)
    loo, ll, info = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mlp, mloo = Vector{Float64}(undef, N), Vector{Float64}(undef, 1)
    wp = weights === nothing ? C_NULL : pointer(weights)
    GC.@preserve weights begin
        rc = linear ?
            ccall((:gpcc_loo_markov_batch, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                   Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                  h.ptr, M, delays, alpha, rho, wp, mu, var, lp, loo, weights === nothing ? C_NULL : pointer(mlp),
                  weights === nothing ? C_NULL : pointer(mloo), ll, info) :
            ccall((:gpcc_loo_batch, LIB), Cint,
                  (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                   Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                  h.ptr, M, delays, alpha, rho, wp, mu, var, lp, loo, weights === nothing ? C_NULL : pointer(mlp),
                  weights === nothing ? C_NULL : pointer(mloo), ll, info)
    end
    rc == 0 || error("gpcc_loo_batch: " * lasterror(h.ptr))
    return mu, var, lp, loo, ll, info, (weights === nothing ? nothing : (mlp, mloo[1]))
end

"posterior_offsets at M rows in LINEAR time (gpcc_posterior_offsets_markov_batch: the offset block of the filter's final state):
(mu_postb L×M, Sigma_postb L×L×M, ll[M], info[M]); columns with info != 0 are NaN.  Needs marginalise_b."
function posterior_offsets_markov_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    mu, Sig = Matrix{Float64}(undef, h.L, M), Array{Float64,3}(undef, h.L, h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_posterior_offsets_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, mu, Sig, ll, info)
    rc == 0 || error("gpcc_posterior_offsets_markov_batch: " * lasterror(h.ptr))
    return mu, Sig, ll, info
end

"objective and its gradient for M triples: (ll[M], grad (2L+1)×M, info[M]); a column of grad is [∂/∂α_1..α_L, ∂/∂ρ, ∂/∂τ_1..τ_L]
in the constrained parameters, NaN where info != 0.  The reference has no gradient: this is the derivative of objective(α, ρ)."
function loglik_grad_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, 2h.L + 1, M)                            # column-major (2L+1)×M == row-major M×(2L+1)
    rc = ccall((:gpcc_loglik_grad_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, info)
    rc == 0 || error("gpcc_loglik_grad_batch: " * lasterror(h.ptr))
    return ll, grad, info
end

"loglik_grad_batch in LINEAR time (gpcc_loglik_grad_markov_batch: the Kalman filter's forward sensitivities, one lane per (row,
parameter), DESIGN 4.17; OU, matern32, matern52): (ll[M], grad (2L+1)×M, info[M]).  ll and info are bitwise loglik_markov_batch's; a
column of grad is NaN where info != 0.  Errors for rbf and for marginalise_b with more than 4 bands."
function loglik_grad_markov(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, 2h.L + 1, M)                            # column-major (2L+1)×M == row-major M×(2L+1)
    rc = ccall((:gpcc_loglik_grad_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, info)
    rc == 0 || error("gpcc_loglik_grad_markov_batch: " * lasterror(h.ptr))
    return ll, grad, info
end

"loglik_markov_batch of M rows that each carry their own NOISE MODEL (gpcc_loglik_noise_markov_batch, DESIGN 4.25; OU, matern32,
matern52): point i of band l of row m has the variance kappa[l, m]^2 σ_i^2 + nu[l, m] -> (ll[M], info[M]).  kappa, nu: L×M, or nothing
(all 1 / all 0: then ll and info are bitwise loglik_markov_batch's).  ll[m] is the value of a fresh handle on the error bars
sqrt(kappa^2 σ^2 + nu); kappa = 0 with one nu for all bands is K + σ²I + B of src/UNUSED/gpccfixdelay_globalnoiseterm.jl:137-147.
info = -3 (after -1, -2): a kappa or nu of the row is negative or not finite."
function loglik_markov_noise(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                             kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_loglik_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, kappa === nothing ? C_NULL : kappa, nu === nothing ? C_NULL : nu, ll, info)
    rc == 0 || error("gpcc_loglik_noise_markov_batch: " * lasterror(h.ptr))
    return ll, info
end

"loglik_markov_noise and its gradient (gpcc_loglik_grad_noise_markov_batch): (ll[M], grad (4L+1)×M, info[M]), a column of grad being
[α_1..α_L, ρ, τ_1..τ_L, kappa_1..kappa_L, nu_1..nu_L]; NaN where info != 0."
function loglik_grad_markov_noise(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                  kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, 4h.L + 1, M)                            # column-major (4L+1)×M == row-major M×(4L+1)
    rc = ccall((:gpcc_loglik_grad_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, kappa === nothing ? C_NULL : kappa, nu === nothing ? C_NULL : nu, ll, grad, info)
    rc == 0 || error("gpcc_loglik_grad_noise_markov_batch: " * lasterror(h.ptr))
    return ll, grad, info
end

"loglik_grad_markov_noise and the Hessian over [α_1..α_L, ρ, kappa_1..kappa_L, nu_1..nu_L] (gpcc_loglik_hess_noise_markov_batch, DESIGN
4.26): (ll[M], grad (4L+1)×M, hess (3L+1)×(3L+1)×M, info[M]); symmetric blocks, NaN where info != 0; ll, grad, info bitwise the gradient's."
function loglik_hess_markov_noise(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                  kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing)
    M, n = length(rho), 3h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad, hess = Matrix{Float64}(undef, 4h.L + 1, M), Array{Float64}(undef, n, n, M)
    rc = ccall((:gpcc_loglik_hess_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, kappa === nothing ? C_NULL : kappa, nu === nothing ? C_NULL : nu, ll, grad, hess, info)
    rc == 0 || error("gpcc_loglik_hess_noise_markov_batch: " * lasterror(h.ptr))
    return ll, grad, hess, info
end

"loglik_grad_markov_noise and the full Hessian, the delays included, over [α_1..α_L, ρ, τ_1..τ_L, kappa_1..kappa_L, nu_1..nu_L]
(gpcc_loglik_hess_full_noise_markov_batch, DESIGN 4.27): (ll[M], grad (4L+1)×M, hess (4L+1)×(4L+1)×M, info[M]); symmetric blocks, NaN
where info != 0; on an OU row with a cross-band tie the entries with a τ index are NaN; ll, grad, info bitwise the gradient's."
function loglik_hess_full_markov_noise(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                       kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing)
    M, n = length(rho), 4h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad, hess = Matrix{Float64}(undef, n, M), Array{Float64}(undef, n, n, M)
    rc = ccall((:gpcc_loglik_hess_full_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, kappa === nothing ? C_NULL : kappa, nu === nothing ? C_NULL : nu, ll, grad, hess, info)
    rc == 0 || error("gpcc_loglik_hess_full_noise_markov_batch: " * lasterror(h.ptr))
    return ll, grad, hess, info
end

# kappa, nu of the four entries below: L×M or nothing (all 1 / all 0), as loglik_markov_noise
_noiseptr(x) = x === nothing ? C_NULL : x

"predict_markov_batch of M rows that each carry their own noise model (gpcc_predict_noise_markov_batch, DESIGN 4.29): column m is what a
fresh handle on the error bars sqrt(kappa[:, m]^2 σ^2 + nu[:, m]) returns -- the latent curve's mean and variance, the noise model
entering through the training points; bitwise predict_markov_batch's at kappa = 1, nu = 0.  info = -3: a kappa or nu negative or not finite."
function predict_markov_noise_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                    ttest::Vector{Vector{Float64}}; kappa::Union{Nothing,Matrix{Float64}} = nothing,
                                    nu::Union{Nothing,Matrix{Float64}} = nothing, weights::Union{Nothing,Vector{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    Nt, tt = Cint.(length.(ttest)), reduce(vcat, ttest)
    T = length(tt)
    mu, var = Matrix{Float64}(undef, T, M), Matrix{Float64}(undef, T, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mm, mv = Vector{Float64}(undef, T), Vector{Float64}(undef, T)
    GC.@preserve weights begin
        rc = ccall((:gpcc_predict_noise_markov_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                   h.ptr, M, delays, alpha, rho, _noiseptr(kappa), _noiseptr(nu), Nt, tt, weights === nothing ? C_NULL : pointer(weights), mu, var,
                   weights === nothing ? C_NULL : pointer(mm), weights === nothing ? C_NULL : pointer(mv), ll, info)
    end
    rc == 0 || error("gpcc_predict_noise_markov_batch: " * lasterror(h.ptr))
    return mu, var, ll, info, (weights === nothing ? nothing : (mm, mv))
end

"heldout_loglik_markov_batch under a per-row noise model (gpcc_heldout_loglik_noise_markov_batch): a test point of band l is scored with
the variance kappa[l, m]^2 σ*^2 + nu[l, m] (+ JITTER), the training points with theirs -> (heldout[M], ll[M], info[M], mix or nothing)."
function heldout_loglik_markov_noise_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                           ttest::Vector{Vector{Float64}}, ytest::Vector{Vector{Float64}}, sigmatest::Vector{Vector{Float64}};
                                           kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing,
                                           weights::Union{Nothing,Vector{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == length(ytest) == length(sigmatest) == h.L
    @assert length.(ttest) == length.(ytest) == length.(sigmatest)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    Nt, tt, yt, st = Cint.(length.(ttest)), reduce(vcat, ttest), reduce(vcat, ytest), reduce(vcat, sigmatest)
    held, ll, info = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mix = Vector{Float64}(undef, 1)
    GC.@preserve weights begin
        rc = ccall((:gpcc_heldout_loglik_noise_markov_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                   h.ptr, M, delays, alpha, rho, _noiseptr(kappa), _noiseptr(nu), Nt, tt, yt, st,
                   weights === nothing ? C_NULL : pointer(weights), held, weights === nothing ? C_NULL : pointer(mix), ll, info)
    end
    rc == 0 || error("gpcc_heldout_loglik_noise_markov_batch: " * lasterror(h.ptr))
    return held, ll, info, (weights === nothing ? nothing : mix[1])
end

"posterior_offsets_markov_batch under a per-row noise model (gpcc_posterior_offsets_noise_markov_batch): (mu_postb L×M, Sigma_postb
L×L×M, ll[M], info[M])."
function posterior_offsets_markov_noise_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64};
                                              kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    mu, Sig = Matrix{Float64}(undef, h.L, M), Array{Float64,3}(undef, h.L, h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_posterior_offsets_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, _noiseptr(kappa), _noiseptr(nu), mu, Sig, ll, info)
    rc == 0 || error("gpcc_posterior_offsets_noise_markov_batch: " * lasterror(h.ptr))
    return mu, Sig, ll, info
end

"loo_batch(linear = true) under a per-row noise model (gpcc_loo_noise_markov_batch): var_i = h'P_s h + kappa_b^2 σ_i^2 + nu_b, so
(y − mu) ./ sqrt.(var) is standardised by the FITTED error bars -> (mu N×M, var N×M, lp N×M, loo[M], ll[M], info[M], mix)."
function loo_markov_noise_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64};
                                kappa::Union{Nothing,Matrix{Float64}} = nothing, nu::Union{Nothing,Matrix{Float64}} = nothing,
                                weights::Union{Nothing,Vector{Float64}} = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    N = Int(ccall((:gpcc_get_option, LIB), Clong, (Ptr{Cvoid}, Cstring), h.ptr, "N"))
    mu, var, lp = Matrix{Float64}(undef, N, M), Matrix{Float64}(undef, N, M), Matrix{Float64}(undef, N, M)
    loo, ll, info = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    mlp, mloo = Vector{Float64}(undef, N), Vector{Float64}(undef, 1)
    GC.@preserve weights begin
        rc = ccall((:gpcc_loo_noise_markov_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
                   h.ptr, M, delays, alpha, rho, _noiseptr(kappa), _noiseptr(nu), weights === nothing ? C_NULL : pointer(weights), mu, var, lp,
                   loo, weights === nothing ? C_NULL : pointer(mlp), weights === nothing ? C_NULL : pointer(mloo), ll, info)
    end
    rc == 0 || error("gpcc_loo_noise_markov_batch: " * lasterror(h.ptr))
    return mu, var, lp, loo, ll, info, (weights === nothing ? nothing : (mlp, mloo[1]))
end

"objective, gradient, Hessian and expected (Fisher) information for M triples: (ll[M], grad (2L+1)×M, hess and fisher
(2L+1)×(2L+1)×M, info[M]) in [α_1..α_L, ρ, τ_1..τ_L] order, symmetric blocks, NaN where info != 0; fisher = 1/2 tr(K⁻¹D_iK⁻¹D_j)."
function loglik_hess_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M, P = length(rho), 2h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, P, M)
    hess, fisher = Array{Float64}(undef, P, P, M), Array{Float64}(undef, P, P, M)   # symmetric: row- or column-major alike
    rc = ccall((:gpcc_loglik_hess_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, hess, fisher, info)
    rc == 0 || error("gpcc_loglik_hess_batch: " * lasterror(h.ptr))
    return ll, grad, hess, fisher, info
end

"the [α_1..α_L, ρ] block of loglik_hess_batch, bitwise its leading (L+1)×(L+1) block: (ll[M], grad (2L+1)×M, hess and fisher
(L+1)×(L+1)×M, info[M]); only that block is formed on the device."
function loglik_hess_hyper_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M, P, n = length(rho), 2h.L + 1, h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, P, M)
    hess, fisher = Array{Float64}(undef, n, n, M), Array{Float64}(undef, n, n, M)   # symmetric: row- or column-major alike
    rc = ccall((:gpcc_loglik_hess_hyper_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, hess, fisher, info)
    rc == 0 || error("gpcc_loglik_hess_hyper_batch: " * lasterror(h.ptr))
    return ll, grad, hess, fisher, info
end

"the [α_1..α_L, ρ] block of the Hessian in LINEAR time (gpcc_loglik_hess_hyper_markov_batch: the Kalman filter's second-order forward
sensitivities, one lane per (row, pair of parameters), DESIGN 4.18; OU, matern32, matern52): (ll[M], grad (2L+1)×M, hess
(L+1)×(L+1)×M, info[M]).  ll, grad and info are bitwise loglik_grad_markov's; hess is bitwise symmetric, NaN where info != 0.  The Fisher
information in linear time: loglik_fisher_markov below; the rows of τ: loglik_hess_markov below.  Errors for rbf, for marginalise_b
with more than 4 bands, and for matern52 with marginalise_b and 4 bands (that instantiation needs scratch memory and does not ship).
The option "laplace_markov" (ccall((:gpcc_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Clong), h.ptr, "laplace_markov", 1)) makes
laplace_evidence's Newton rounds call this entry."
function loglik_hess_hyper_markov(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M, P, n = length(rho), 2h.L + 1, h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, P, M)
    hess = Array{Float64}(undef, n, n, M)                                 # symmetric: row- or column-major alike
    rc = ccall((:gpcc_loglik_hess_hyper_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, hess, info)
    rc == 0 || error("gpcc_loglik_hess_hyper_markov_batch: " * lasterror(h.ptr))
    return ll, grad, hess, info
end

"the FULL Hessian over [α_1..α_L, ρ, τ_1..τ_L] in LINEAR time (gpcc_loglik_hess_markov_batch: the same second-order forward
sensitivities with the tangents of the transition by the lags, one lane per (row, pair), DESIGN 4.21; OU, matern32, matern52):
(ll[M], grad (2L+1)×M, hess (2L+1)×(2L+1)×M, info[M]).  ll, grad and info are bitwise loglik_grad_markov's and the leading (L+1)×(L+1)
block bitwise loglik_hess_hyper_markov's; hess is bitwise symmetric, NaN where info != 0.  OU has no second derivative by τ on a row
where two points of different bands have exactly equal shifted times: there every entry with a τ index is NaN, info stays 0 and the
rest is untouched -- use loglik_hess_batch for OU on a grid of delays that collides with the cadence.  The Matérn kernels are exact
at ties.  The Fisher information in linear time: loglik_fisher_markov.  Errors as loglik_hess_hyper_markov."
function loglik_hess_markov(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M, P = length(rho), 2h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, P, M)
    hess = Array{Float64}(undef, P, P, M)                                 # symmetric: row- or column-major alike
    rc = ccall((:gpcc_loglik_hess_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, hess, info)
    rc == 0 || error("gpcc_loglik_hess_markov_batch: " * lasterror(h.ptr))
    return ll, grad, hess, info
end

"the expected (FISHER) information over [α_1..α_L, ρ, τ_1..τ_L] in LINEAR time (gpcc_loglik_fisher_markov_batch: the Kalman filter
carrying the second moments of its means and of their tangents, one lane per (row, pair), DESIGN 4.22; OU, matern32, matern52):
(ll[M], grad (2L+1)×M, fisher (2L+1)×(2L+1)×M, info[M]).  ll, grad and info are bitwise loglik_grad_markov's; fisher is bitwise
symmetric, NaN where info != 0, positive semi-definite at any point, and reads the fluxes through the offsets' prior variances only.
On an OU row where two points of different bands have exactly equal shifted times every entry with a τ index is NaN, info stays 0 and
the (α, ρ) block is exact -- use loglik_hess_batch's fisher there.  The Matérn kernels are exact at ties.  Errors for rbf, for
marginalise_b with more than 4 bands, and for matern52 with marginalise_b and 4 bands (that instantiation does not ship)."
function loglik_fisher_markov(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64})
    M, P = length(rho), 2h.L + 1
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    grad = Matrix{Float64}(undef, P, M)
    fisher = Array{Float64}(undef, P, P, M)                               # symmetric: row- or column-major alike
    rc = ccall((:gpcc_loglik_fisher_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, ll, grad, fisher, info)
    rc == 0 || error("gpcc_loglik_fisher_markov_batch: " * lasterror(h.ptr))
    return ll, grad, fisher, info
end

"the log-likelihood of R flux realisations per column (τ, α, ρ) in ONE linear-time pass (gpcc_loglik_markov_multi_batch: per column the
filter's covariance recursion runs once and drives R means, DESIGN 4.23; OU, matern32, matern52) -> (ll R×M, info[M]).  Y: N×R, column
r one realisation in the order the handle took y.  mean: L×R, the offset subtracted per realisation and band, or nothing: the handle's
band means.  The model is the handle's: times, σ, kernel, b-mode and, with marginalise_b, the prior variances of the y it was created
with.  info is loglik_markov's and depends on the column (τ, α, ρ) only; such a column is NaN for every realisation; a flux that is
not finite makes its own realisation NaN.  Errors for rbf and for marginalise_b with more than 4 bands."
function loglik_markov_realisations(h::Handle, Y::Matrix{Float64}, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64};
                                    mean = nothing)
    M, R = length(rho), size(Y, 2)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && R >= 1
    @assert mean === nothing || size(mean) == (h.L, R)
    ll, info = Matrix{Float64}(undef, R, M), Vector{Cint}(undef, M)         # C writes M×R row-major: R×M here
    rc = ccall((:gpcc_loglik_markov_multi_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, R, Y, mean === nothing ? C_NULL : convert(Matrix{Float64}, mean), ll, info)
    rc == 0 || error("gpcc_loglik_markov_multi_batch: " * lasterror(h.ptr))
    return ll, info
end

"the log-likelihood of M columns (τ, α, ρ) that each carry THEIR OWN RESAMPLED DATA SET on the handle's cadence, in one linear-time pass
(gpcc_loglik_markov_resampled_batch, DESIGN 4.24; OU, matern32, matern52) -> (ll[M], info[M]): flux randomisation with a refit per
realisation, random subset selection, each realisation's own Σ_b.  Y: N×R, column r one realisation in the order the handle took y.
real[m] in 1:R: the realisation of column m.  counts: N×R multiplicities ≥ 0 (0 drops the point, n > 1 is the point once with σ²/n) or
nothing: all 1.  mean, sigma_b: L×R -- each realisation's band means and offsets' prior variances (for the value of a fresh handle on
the kept points: the means and 100 var (n - 1) of its distinct kept points) -- or nothing: the handle's.  A realisation that keeps no
point gives 0.0.  info is loglik_markov's, a positive value counted among the kept points.  A flux that is not finite at a kept point
makes the columns of that realisation NaN.  Errors for rbf, for marginalise_b with more than 4 bands, and for a call whose packed data
(16 N R bytes) exceeds the option markov_resample_bytes_max: split R."
function loglik_markov_resampled(h::Handle, Y::Matrix{Float64}, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                 real::Vector{<:Integer}; counts = nothing, mean = nothing, sigma_b = nothing)
    M, R = length(rho), size(Y, 2)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(real) == M && R >= 1
    @assert all(1 .<= real .<= R)
    @assert counts === nothing || (size(counts) == size(Y) && all(counts .>= 0))
    @assert mean === nothing || size(mean) == (h.L, R)
    @assert sigma_b === nothing || size(sigma_b) == (h.L, R)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_loglik_markov_resampled_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, convert(Vector{Cint}, real .- 1), R, Y,
               counts === nothing ? C_NULL : convert(Matrix{Cint}, counts), mean === nothing ? C_NULL : convert(Matrix{Float64}, mean),
               sigma_b === nothing ? C_NULL : convert(Matrix{Float64}, sigma_b), ll, info)
    rc == 0 || error("gpcc_loglik_markov_resampled_batch: " * lasterror(h.ptr))
    return ll, info
end

"loglik_markov_resampled and its exact gradient in linear time (gpcc_loglik_grad_markov_resampled_batch, DESIGN 4.28) ->
(ll[M], grad (2L+1)×M, info[M]), column m of grad = [∂/∂α_1..L, ∂/∂ρ, ∂/∂τ_1..L] of ll[m]: the gradient of a fresh handle on the kept
points of realisation real[m], the band means and Σ_b being constants of the data.  The arguments and errors are
loglik_markov_resampled's; ll and info are bitwise its results.  A column with info ≠ 0 is NaN; a realisation that keeps no point gives
0.0 and a zero gradient; OU at an exact tie between two kept points of different bands returns the mean of the one-sided derivatives."
function loglik_grad_markov_resampled(h::Handle, Y::Matrix{Float64}, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64},
                                      real::Vector{<:Integer}; counts = nothing, mean = nothing, sigma_b = nothing)
    M, R = length(rho), size(Y, 2)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(real) == M && R >= 1
    @assert all(1 .<= real .<= R)
    @assert counts === nothing || (size(counts) == size(Y) && all(counts .>= 0))
    @assert mean === nothing || size(mean) == (h.L, R)
    @assert sigma_b === nothing || size(sigma_b) == (h.L, R)
    ll, grad, info = Vector{Float64}(undef, M), Matrix{Float64}(undef, 2 * h.L + 1, M), Vector{Cint}(undef, M)
    rc = ccall((:gpcc_loglik_grad_markov_resampled_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, convert(Vector{Cint}, real .- 1), R, Y,
               counts === nothing ? C_NULL : convert(Matrix{Cint}, counts), mean === nothing ? C_NULL : convert(Matrix{Float64}, mean),
               sigma_b === nothing ? C_NULL : convert(Matrix{Float64}, sigma_b), ll, grad, info)
    rc == 0 || error("gpcc_loglik_grad_markov_resampled_batch: " * lasterror(h.ptr))
    return ll, grad, info
end

"Laplace-marginalised evidence over α and ρ per delay (columns of delays, L×G), from (alpha0 L×G, rho0[G]), usually the fit's
output.  Prior log-uniform in α and in ρ on [rhomin, rhomax]: log_evidence is log Z(τ) up to ONE additive constant shared by all
delays -- use it only through getprobabilities (or differences).  -> (ll[G], alpha L×G, rho[G], log_evidence[G], cov (L+1)×(L+1)×G
of (log α, log ρ), info[G]: 0, -10 not converged, -11 not a maximum, -12 mode on the ρ bound, or the start's own code; rounds[G])."
function laplace_evidence(h::Handle, delays::Matrix{Float64}, alpha0::Matrix{Float64}, rho0::Vector{Float64};
                          rhomin = 0.1, rhomax = 20.0, max_rounds = 50, g_tol = 1e-6)
    G, n = length(rho0), h.L + 1
    @assert size(delays) == (h.L, G) && size(alpha0) == (h.L, G)
    ll, alpha, rho = Vector{Float64}(undef, G), Matrix{Float64}(undef, h.L, G), Vector{Float64}(undef, G)
    logz, cov = Vector{Float64}(undef, G), Array{Float64}(undef, n, n, G)   # symmetric: row- or column-major alike
    info, rounds = Vector{Cint}(undef, G), Vector{Cint}(undef, G)
    rc = ccall((:gpcc_laplace_evidence, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cint, Cdouble, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Clonglong}),
               h.ptr, G, delays, alpha0, rho0, rhomin, rhomax, max_rounds, g_tol, ll, alpha, rho, logz, cov, info, rounds, C_NULL)
    rc == 0 || error("gpcc_laplace_evidence: " * lasterror(h.ptr))
    return ll, alpha, rho, logz, cov, info, rounds
end

"posterior predictive at the columns (τ, α, ρ) of delays, alpha (L×M) and rho[M] on test times shared by all of them (ttest: L
vectors), and its average over the columns with weights (M, or nothing) -> (mu T×M, var T×M (the diagonal of predict's Σ, JITTER
included), ll[M], info[M] (bitwise loglik_grad_batch's; NaN columns where info != 0), mix_mu[T], mix_var[T] (nothing without weights)).
mix_mu = Σ p μ, mix_var = Σ p (var + (μ - mix_mu)²), p = weights / sum(weights); a mixture of Gaussians has no joint covariance."
function predict_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64}, ttest; weights = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    Nt = Cint[length(a) for a in ttest]
    tt = Float64.(reduce(vcat, ttest))
    T = length(tt)
    mu, var = Matrix{Float64}(undef, T, M), Matrix{Float64}(undef, T, M)   # column-major T×M == row-major M×T
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    w = weights === nothing ? C_NULL : Float64.(weights)
    mm, mv = weights === nothing ? (C_NULL, C_NULL) : (Vector{Float64}(undef, T), Vector{Float64}(undef, T))
    rc = ccall((:gpcc_predict_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, Nt, tt, w, mu, var, mm, mv, ll, info)
    rc == 0 || error("gpcc_predict_batch: " * lasterror(h.ptr))
    return mu, var, ll, info, (weights === nothing ? nothing : mm), (weights === nothing ? nothing : mv)
end

"held-out log-likelihood of the test set (ttest, ytest, σtest: L vectors each, shared by every column) at the columns (τ, α, ρ) of
delays, alpha (L×M) and rho[M], and its average over the columns with weights (M, or nothing) -> (heldout[M] (predictTest(ttest, ytest,
σtest), marginaliseb.jl:311-325), ll[M] (bitwise loglik_grad_batch's), info[M] (N + j: the j-th pivot of the test block failed; heldout
NaN, ll valid), mix (log Σ p exp(heldout), p = weights / sum(weights); nothing without weights)).  The nearestposdef retry of :327-341
is left to the caller (rows with info > N)."
function heldout_loglik_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64}, ttest, ytest, σtest;
                              weights = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == length(ytest) == length(σtest) == h.L
    @assert all(length.(ttest) .== length.(ytest) .== length.(σtest))
    Nt = Cint[length(a) for a in ttest]
    tt, yt, st = Float64.(reduce(vcat, ttest)), Float64.(reduce(vcat, ytest)), Float64.(reduce(vcat, σtest))
    held, ll, info = Vector{Float64}(undef, M), Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    w = weights === nothing ? C_NULL : Float64.(weights)
    mix = weights === nothing ? C_NULL : Vector{Float64}(undef, 1)
    rc = ccall((:gpcc_heldout_loglik_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, Nt, tt, yt, st, w, held, mix, ll, info)
    rc == 0 || error("gpcc_heldout_loglik_batch: " * lasterror(h.ptr))
    return held, ll, info, (weights === nothing ? nothing : mix[1])
end

"joint posterior draws of the light curves on the test times ttest (L vectors, shared by every column) at the columns (τ, α, ρ) of
delays, alpha (L×M) and rho[M]: f* = μpred + chol(Σpred + JITTER I + diag(σtest²)) ζ (σtest = nothing: the latent curve) ->
(draws (T × D), draw_row[D], ll[M], info[M], ζ (T × D) or nothing).  weights = nothing: D = M S, draw s of column m in column m S + s;
weights (M): D = S draws of the mixture, draw_row the 0-based column each used (columns without a draw: ll NaN, info -14).  ll and info
are heldout_loglik_batch's (info = N + j: the j-th pivot of the test block failed, draws NaN).  seed: the Philox4x64-10 key."
function sample_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64}, ttest, S::Integer, seed::Integer;
                      weights = nothing, σtest = nothing, return_noise::Bool = false)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    Nt = Cint[length(a) for a in ttest]
    tt = Float64.(reduce(vcat, ttest))
    T = length(tt)
    st = σtest === nothing ? C_NULL : Float64.(reduce(vcat, σtest))
    D = weights === nothing ? M * S : S
    draws, rows = Matrix{Float64}(undef, T, D), Vector{Cint}(undef, D)
    ζ = return_noise ? Matrix{Float64}(undef, T, D) : C_NULL
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    w = weights === nothing ? C_NULL : Float64.(weights)
    rc = ccall((:gpcc_sample_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                Culonglong, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, Nt, tt, st, w, S, UInt64(seed), draws, rows, ζ, ll, info)
    rc == 0 || error("gpcc_sample_batch: " * lasterror(h.ptr))
    return draws, rows, ll, info, (return_noise ? ζ : nothing)
end

"sample_batch in LINEAR time for OU, matern32 and matern52 (gpcc_sample_markov_batch: Matheron's rule over the Kalman filter, O(N + T) per
draw, no T×T factor): the same distribution N(μpred, Σpred + JITTER I + diag(σtest²)), other draws -> (draws (T × D), draw_row[D], ll[M],
info[M]) in sample_batch's layouts and modes.  draw_row is sample_batch's for the same seed and weights; ll and info of a drawn column
are predict_markov_batch's (draws NaN where info != 0); columns without a draw: ll NaN, info -14."
function sample_markov_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64}, ttest, S::Integer,
                             seed::Integer; weights = nothing, σtest = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    Nt = Cint[length(a) for a in ttest]
    tt = Float64.(reduce(vcat, ttest))
    T = length(tt)
    st = σtest === nothing ? C_NULL : Float64.(reduce(vcat, σtest))
    D = weights === nothing ? M * S : S
    draws, rows = Matrix{Float64}(undef, T, D), Vector{Cint}(undef, D)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    w = weights === nothing ? C_NULL : Float64.(weights)
    rc = ccall((:gpcc_sample_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                Culonglong, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, Nt, tt, st, w, S, UInt64(seed), draws, rows, ll, info)
    rc == 0 || error("gpcc_sample_markov_batch: " * lasterror(h.ptr))
    return draws, rows, ll, info
end

"sample_markov_batch of M columns that each carry their own noise model (gpcc_sample_noise_markov_batch, DESIGN 4.30): kappa, nu L×M or
nothing (all 1 / all 0).  Column m's draws are, to rounding and with the SAME seed, those of a fresh handle on the error bars
sqrt(kappa[:, m]^2 σ^2 + nu[:, m]): with σtest a test point of band l is a replicated observation of variance JITTER + kappa[l, m]^2
σtest^2 + nu[l, m], without it the latent curve (noise variance JITTER: nu is not added; σtest of zeros asks for the curve plus the
excess variance).  draw_row is sample_markov_batch's for the same seed and weights; bitwise sample_markov_batch's at kappa = 1, nu = 0;
ll and info of a drawn column are predict_markov_noise_batch's, info = -3 (a kappa or nu negative or not finite) makes its draws NaN."
function sample_markov_noise_batch(h::Handle, delays::Matrix{Float64}, alpha::Matrix{Float64}, rho::Vector{Float64}, ttest, S::Integer,
                                   seed::Integer; kappa::Union{Nothing,Matrix{Float64}} = nothing,
                                   nu::Union{Nothing,Matrix{Float64}} = nothing, weights = nothing, σtest = nothing)
    M = length(rho)
    @assert size(delays) == (h.L, M) && size(alpha) == (h.L, M) && length(ttest) == h.L
    @assert (kappa === nothing || size(kappa) == (h.L, M)) && (nu === nothing || size(nu) == (h.L, M))
    Nt = Cint[length(a) for a in ttest]
    tt = Float64.(reduce(vcat, ttest))
    T = length(tt)
    st = σtest === nothing ? C_NULL : Float64.(reduce(vcat, σtest))
    D = weights === nothing ? M * S : S
    draws, rows = Matrix{Float64}(undef, T, D), Vector{Cint}(undef, D)
    ll, info = Vector{Float64}(undef, M), Vector{Cint}(undef, M)
    w = weights === nothing ? C_NULL : Float64.(weights)
    rc = ccall((:gpcc_sample_noise_markov_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Cint, Culonglong, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cint}),
               h.ptr, M, delays, alpha, rho, _noiseptr(kappa), _noiseptr(nu), Nt, tt, st, w, S, UInt64(seed), draws, rows, ll, info)
    rc == 0 || error("gpcc_sample_noise_markov_batch: " * lasterror(h.ptr))
    return draws, rows, ll, info
end

"Drop-in body of objective(α, ρ) (gpccfixdelay_marginaliseb.jl:133-141): throws what the Julia code throws."
function objective(h::Handle, τ, α, ρ)
    ll, info = loglik_batch(h, reshape(Float64.(τ), :, 1), reshape(Float64.(α), :, 1), [Float64(ρ)])
    info[1] == -1 && throw(AssertionError("all(scale .> 0)"))            # delayedCovariance.jl:3
    info[1] == -2 && error("ρ=$(ρ) is <= 0")                             # delayedCovariance.jl:5-7
    info[1] >  0 && throw(LinearAlgebra.PosDefException(info[1]))        # cholesky inside MvNormal, :139
    return ll[1]
end

"""
The whole README sweep `map(d -> gpcc(...; delays = [0; d])[1], candidatedelays)` (README.md:172-174) as one call.
`delays` is L×G.  The random candidates are drawn HERE exactly as gpccfixdelay_marginaliseb.jl:160-196 draws them
(same MersenneTwister(seed), same order), so every delay starts where the reference starts it.
"""
function grid_loglik(h::Handle, delays::Matrix{Float64}, yarray; iterations, seed = 1, numberofrestarts = 1,
                     initialrandom = 5, rhomin = 0.1, rhomax)
    L, G = size(delays)
    rg = MersenneTwister(seed)                                                   # :62
    initialρ = numberofrestarts <= 2 ? rand(rg, Uniform(rhomin + 1e-3, rhomax - 1e-3), numberofrestarts) :
                                        collect(MiscUtil.logrange(rhomin + 1e-3, rhomax - 1e-3, numberofrestarts))
    init = Array{Float64}(undef, L + 1, initialrandom, numberofrestarts)        # column-major == R×C×(L+1) row-major
    for i in 1:numberofrestarts, c in 1:initialrandom
        α = map(var, yarray) .* (rand(rg, L) * (1.2 - 0.8) .+ 0.8)             # sampleα, :188
        init[:, c, i] = [invmakepositive.(α); invtransformbetween(initialρ[i], rhomin, rhomax)]   # :195-196
    end
    ll, ρ, info = Vector{Float64}(undef, G), Vector{Float64}(undef, G), Vector{Cint}(undef, G)
    α = Matrix{Float64}(undef, L, G)
    rc = ccall((:gpcc_grid_loglik, LIB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Cint, Cint, Cdouble, Cdouble, Culonglong, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Clonglong}),
               h.ptr, G, delays, iterations, numberofrestarts, initialrandom, rhomin, rhomax, seed, init,
               ll, α, ρ, info, C_NULL, C_NULL)
    rc == 0 || error("gpcc_grid_loglik: " * lasterror(h.ptr))
    return ll, α, ρ, info
end

"getprobabilities(loglikel[, logprior]) (getprobabilities.jl:1-20); same shape as the input."
function probabilities(loglikel::Array{Float64}, logprior = nothing; device = 0)
    out = similar(loglikel)
    lp  = logprior === nothing ? C_NULL : Float64.(vec(logprior))        # ccall roots the array for the call
    rc = ccall((:gpcc_probabilities, LIB), Cint, (Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint),
               length(loglikel), loglikel, lp, out, device)
    rc == 0 || error("gpcc_probabilities: " * lasterror(C_NULL))
    return out
end

end # module

# ExtendedRtIrtModelingAMD.jl -- Julia-side drop-in for the `sample!` hot path of ExtendedRtIrtModeling.jl, backed by
# libertirt.so (include/ertirt.h).  SHIPS AS SOURCE, UNTESTED: no Julia toolchain exists in the build container or on
# the GPU box (SURVEY.md 8(b)); the same C ABI is exercised by the Python ctypes host in this package, whose tests are
# the parity tests.  See INTEGRATION.md for how a maintainer wires this into the reference package.
#
# What it replaces (paths relative to the reference repository):
#   sample!(::GibbsMlIrt)          src/GibbsRtIrt.pl.jl:210-257
#   sample!(::GibbsRtIrt)          src/GibbsRtIrt.pl.jl:278-346
#   sample!(::GibbsRtIrtCrossQr)   src/GibbsRtIrtCross.pl.jl:265-325
#   sample!(::GibbsRtIrtLatentQr)  src/GibbsRtIrtLatent.pl.jl:271-337
#   sample!(::GibbsRtIrtNull)      src/GibbsRtIrt.pl.jl:367-426
#   sample!(::GibbsRtIrtCross)     src/GibbsRtIrtCross.pl.jl:176-235
#   sample!(::GibbsRtIrtLatent)    src/GibbsRtIrtLatent.pl.jl:168-233
# Struct names, fields, constructor behaviour, kwargs, error text and the Post layout are the reference's; coef / precis /
# getDic / comparePara / checkConvergence of the reference keep working on the filled `Post`.
module ExtendedRtIrtModelingAMD

using LinearAlgebra, Random

export sample!, GibbsMlIrt, GibbsRtIrt, GibbsRtIrtCrossQr, GibbsRtIrtLatentQr, GibbsRtIrtQuantile, GibbsRtIrtNull, GibbsRtIrtCross,
       GibbsRtIrtLatent, essRhat, rankEssRhat, rankEssRhatDraws, simulateData!, libertirt_path!, rcclUniqueId, getDicDevice, getWaicDevice, getWaicMarginal, marginalLogLik, getWaicMarginalQr, getLooMarginalQr, quantileMarginalLogLik, getScores, scoreRespondents, getPersonFit, personFit, getItemFit, itemFit, getPlausibleValues, drawPlausibleValues, observedMask, getLooMarginal, psisLoo, setPointwise!, getPpcDevice, setPredictive!, checkConvergenceDevice, setSeed!

const LIB = Ref{String}(get(ENV, "LIBERTIRT", "libertirt.so"))
libertirt_path!(p::AbstractString) = (LIB[] = String(p))
# the 128-byte ncclUniqueId of a subject-sharded chain: made on ONE process, handed to all of them (MPI.Bcast!, a file, ...)
rcclUniqueId() = (u = zeros(UInt8, 128); check(ccall((:erm_rccl_unique_id, LIB[]), Cint, (Ptr{UInt8},), u)); u)

# ---- mirror of erm_config / erm_state / erm_timing (include/ertirt.h); field order and types must match exactly
struct ErmConfig
    model::Int32; n_item::Int32; n_subj::Int64; n_feat::Int32; n_iter::Int32; n_chain::Int32; n_burnin::Int32
    intercept::Int32; one_pl::Int32; cov2one::Int32; sigp_mode::Int32; chain_id::Int32; q_rt::Float64; seed::UInt64
    device::Int32; precision::Int32; trace_mode::Int32; lanes_per_row::Int32; block_threads::Int32; grid_blocks::Int32
    profile::Int32; flags::Int32; nu_trace_max_gb::Float64
end
struct ErmState
    theta::Ptr{Float64}; a::Ptr{Float64}; b::Ptr{Float64}; zeta::Ptr{Float64}; lambda::Ptr{Float64}; sig2t::Ptr{Float64}
    beta::Ptr{Float64}; sigp::Ptr{Float64}; rho::Ptr{Float64}; nu::Ptr{Float64}
end
# (the per-model widths below -- nb, nnu, which models read X or have rt / ρ -- restate the table of csrc/erm_model.hpp and _lib.py's MODEL_TRAITS)
const MODEL_MLIRT, MODEL_RTIRT, MODEL_CROSSQR, MODEL_LATENTQR = Int32(0), Int32(1), Int32(2), Int32(3)
const MODEL_NULL, MODEL_CROSS, MODEL_LATENT = Int32(4), Int32(5), Int32(6)
const TRACE_RA, TRACE_RT, TRACE_QR, TRACE_LOGLIKE = Int32(0), Int32(1), Int32(2), Int32(3)

lasterr() = unsafe_string(ccall((:erm_last_error, LIB[]), Cstring, ()))
check(rc::Integer) = rc == 0 ? nothing : error("libertirt: " * lasterr())
# the struct mirrors above were written against ERM_ABI_VERSION 4 of include/ertirt.h
const ABI_VERSION = 4
function checkAbi()
    v = ccall((:erm_abi_version, LIB[]), Cint, ())
    v == ABI_VERSION || error("libertirt: the library's struct layout version is $v, this module was written against $ABI_VERSION")
end

# ---- the reference's containers (src/Base.pl.jl:100-115), reproduced so the module is self-contained when used stand-alone;
# inside the reference package these definitions are simply dropped in favour of the existing ones.
Base.@kwdef mutable struct InputPara
    ω::Array = Float64[]; θ::Array = Float64[]; a::Array = Float64[]; b::Array = Float64[]; ζ::Array = Float64[]
    λ::Array = Float64[]; σ²t::Array = Float64[]; ν::Array = Float64[]; β::Array = Float64[]; ρ::Array = Float64[]; Σp::Array = Float64[]
end
mutable struct OutputPost
    ra; rt; qr; logLike; mean
end

abstract type GibbsAMD end
for (T, model) in ((:GibbsMlIrt, MODEL_MLIRT), (:GibbsRtIrt, MODEL_RTIRT), (:GibbsRtIrtCrossQr, MODEL_CROSSQR), (:GibbsRtIrtLatentQr, MODEL_LATENTQR),
                   (:GibbsRtIrtNull, MODEL_NULL), (:GibbsRtIrtCross, MODEL_CROSS), (:GibbsRtIrtLatent, MODEL_LATENT))
    @eval begin
        mutable struct $T <: GibbsAMD
            Cond; Data; truePara; Para; Post
            handle::Ptr{Cvoid}; key::Any; seed::UInt64; device::Int32; precision::Int32
            shard::Any      # nothing, or (rank, count, nSubjTotal, rowBase, uid): Cond.nSubj / Data then describe this process's subjects only
                            # (give every rank the same β / ρ / Σp start, e.g. Random.seed!(s) before the constructor and cut θ, ζ afterwards:
                            #  setInitialValues draws them from the global RNG as the reference does)
            farm::Ptr{Cvoid}   # the chain farm of the last sample!(...; devices), kept until the next sample! (or the finalizer) for checkConvergenceDevice; else C_NULL
            function $T(Cond; Data = [], truePara = [], Para = Float64[], Post = Float64[], seed = 1234, device = 0, precision = 1, shard = nothing)
                obj = new(Cond, Data, truePara, Para, Post, C_NULL, nothing, UInt64(seed), Int32(device), Int32(precision), shard, C_NULL)
                setInitialValues(obj)                      # always overwrites Para, as the reference's constructors do
                obj.Post = OutputPost([], [], [], [], Float64[])
                finalizer(o -> (o.handle != C_NULL && ccall((:erm_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), o.handle); releaseFarm!(o)), obj)
                return obj
            end
        end
        modelid(::$T) = $model
    end
end
const GibbsRtIrtQuantile = GibbsRtIrtLatentQr     # README.md:22,95; the reference's export is commented out (src/ExtendedRtIrtModeling.jl:65)

# setInitialValues: src/GibbsRtIrt.pl.jl:84-93,122-133; src/GibbsRtIrtCross.pl.jl:123-134; src/GibbsRtIrtLatent.pl.jl:113-124
function setInitialValues(s::GibbsMlIrt)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), β = randn(C.nFeat + 1)); s
end
function setInitialValues(s::GibbsRtIrt)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), β = randn(C.nFeat + 1, 2), Σp = Matrix{Float64}(I, 2, 2)); s
end
function setInitialValues(s::GibbsRtIrtCrossQr)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), ρ = randn(C.nItem), Σp = Matrix{Float64}(I, 2, 2)); s
end
function setInitialValues(s::GibbsRtIrtLatentQr)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), β = randn(C.nFeat + 2), Σp = Matrix{Float64}(I, 2, 2)); s
end

# src/GibbsRtIrt.pl.jl:159-170; src/GibbsRtIrtCross.pl.jl:85-96; src/GibbsRtIrtLatent.pl.jl:78-89
function setInitialValues(s::GibbsRtIrtNull)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), Σp = Matrix{Float64}(I, 2, 2)); s
end
function setInitialValues(s::GibbsRtIrtCross)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), ρ = randn(C.nItem), Σp = Matrix{Float64}(I, 2, 2)); s
end
function setInitialValues(s::GibbsRtIrtLatent)
    C = s.Cond
    s.Para = InputPara(θ = randn(C.nSubj), a = ones(C.nItem), b = zeros(C.nItem), ζ = randn(C.nSubj), λ = zeros(C.nItem),
                       σ²t = ones(C.nItem), β = randn(C.nFeat + 2), Σp = Matrix{Float64}(I, 2, 2)); s
end

dense(x) = isempty(x) ? Float64[] : Array{Float64}(x)
ptr(x::Array{Float64}) = isempty(x) ? Ptr{Float64}(C_NULL) : pointer(x)

function engine!(M::GibbsAMD, intercept::Bool, onepl::Bool, cov2one::Bool; upload::Bool = true)
    key = (intercept, onepl, cov2one)
    M.handle != C_NULL && M.key == key && return M.handle
    M.handle != C_NULL && ccall((:erm_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), M.handle)
    C = M.Cond
    cfg = ErmConfig(modelid(M), C.nItem, C.nSubj, C.nFeat, C.nIter, C.nChain, C.nBurnin, intercept, onepl, cov2one, 0, 0, C.qRt,
                    M.seed, M.device, M.precision, 1, 0, 0, 0, 0, 0, 0.0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    checkAbi()
    check(ccall((:erm_create, LIB[]), Cint, (Ref{ErmConfig}, Ref{Ptr{Cvoid}}), cfg, h))
    if M.shard !== nothing       # one chain over several devices (include/ertirt.h, erm_set_shard_rccl): collective, before the data
        rank, count, ntot, base, uid = M.shard
        length(uid) == 128 || error("shard: uid must be the 128 bytes of rcclUniqueId()")
        GC.@preserve uid check(ccall((:erm_set_shard_rccl, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{UInt8}), h[], rank, count, ntot, base, uid))
    end
    if !upload                                                  # the data set will be generated on the device (simulateData!)
        M.handle, M.key = h[], key
        return M.handle
    end
    Y = Array{UInt8}(M.Data.Y)                                  # Matrix{Bool} from setData* or a 0/1 numeric matrix
    logT = modelid(M) == MODEL_MLIRT ? Float64[] : dense(M.Data.logT)
    X = (modelid(M) in (MODEL_CROSSQR, MODEL_CROSS, MODEL_NULL) || C.nFeat == 0) ? Float64[] : dense(M.Data.X)
    GC.@preserve Y logT X check(ccall((:erm_set_data, LIB[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}), h[], Y, ptr(logT), ptr(X)))
    M.handle, M.key = h[], key
    return M.handle
end

function state_arrays(P::InputPara)
    (dense(P.θ), dense(P.a), dense(P.b), dense(P.ζ), dense(P.λ), dense(P.σ²t), dense(vec(P.β)), dense(vec(P.Σp)), dense(P.ρ), dense(vec(P.ν)))
end

# the chain farm a sampler keeps from its last sample!(...; devices): released before the next sample! and by the finalizer
function releaseFarm!(M)
    M.farm != C_NULL && ccall((:erm_farm_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), M.farm)
    M.farm = C_NULL
    return M
end

# nChain INDEPENDENT chains, chain l on GPU devices[l] (erm_farm_*, include/ertirt.h): the library samples them concurrently (one host
# thread per chain) and reduces Post.mean over the devices with one RCCL all-reduce.  Chain 1 starts from MCMC.Para, chain l > 1 from a
# fresh setInitialValues draw, as nChain separately constructed samplers would.
function sampleFarm!(M::GibbsAMD, intercept::Bool, onepl::Bool, cov2one::Bool, devices)
    C = M.Cond
    M.shard === nothing || error("a subject-sharded sampler cannot also farm chains")
    releaseFarm!(M)
    devs = Int32[devices[mod1(l, length(devices))] for l in 1:C.nChain]
    cfg = ErmConfig(modelid(M), C.nItem, C.nSubj, C.nFeat, C.nIter, 1, C.nBurnin, intercept, onepl, cov2one, 0, 0, C.qRt,
                    M.seed, 0, M.precision, 1, 0, 0, 0, 0, 0, 0.0)
    f = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:erm_farm_create, LIB[]), Cint, (Ref{ErmConfig}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}), cfg, devs, C.nChain, f))
    try
        Y = Array{UInt8}(M.Data.Y)
        logT = modelid(M) == MODEL_MLIRT ? Float64[] : dense(M.Data.logT)
        X = (modelid(M) in (MODEL_CROSSQR, MODEL_CROSS, MODEL_NULL) || C.nFeat == 0) ? Float64[] : dense(M.Data.X)
        GC.@preserve Y logT X check(ccall((:erm_farm_set_data, LIB[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}), f[], Y, ptr(logT), ptr(X)))
        first = M.Para
        for l in 1:C.nChain
            l > 1 && setInitialValues(M)                     # a fresh draw for every further chain
            arrs = state_arrays(M.Para)
            GC.@preserve arrs check(ccall((:erm_farm_set_state, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ref{ErmState}), f[], l - 1, ErmState(map(ptr, arrs)...)))
        end
        M.Para = first
        check(ccall((:erm_farm_run, LIB[]), Cint, (Ptr{Cvoid}, Int64), f[], C.nIter))
        h0 = ccall((:erm_farm_engine, LIB[]), Ptr{Cvoid}, (Ptr{Cvoid}, Int32), f[], 0)
        trace(which) = begin
            w = ccall((:erm_trace_width, LIB[]), Int64, (Ptr{Cvoid}, Cint), h0, which)
            out = Array{Float64}(undef, C.nIter, w, C.nChain)
            check(ccall((:erm_farm_get_trace, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), f[], which, out)); out
        end
        Post = M.Post
        Post.ra = trace(TRACE_RA)
        Post.logLike = trace(TRACE_LOGLIKE)
        modelid(M) != MODEL_MLIRT && (Post.rt = trace(TRACE_RT))
        Post.qr = trace(TRACE_QR)
        N, J, F = C.nSubj, C.nItem, C.nFeat
        nb = modelid(M) == MODEL_MLIRT ? F + 1 : modelid(M) in (MODEL_RTIRT, MODEL_NULL) ? 2 * (F + 1) : modelid(M) in (MODEL_LATENTQR, MODEL_LATENT) ? F + 2 : 0
        nnu = modelid(M) == MODEL_LATENTQR ? N : modelid(M) == MODEL_CROSSQR ? N * J : 0
        bufs = (zeros(N), zeros(J), zeros(J), zeros(N), zeros(J), zeros(J), zeros(nb), zeros(4), zeros(J), zeros(nnu))
        GC.@preserve bufs check(ccall((:erm_farm_get_mean, LIB[]), Cint, (Ptr{Cvoid}, Ref{ErmState}), f[], ErmState(map(ptr, bufs)...)))
        Post.mean = InputPara(θ = bufs[1], a = bufs[2], b = bufs[3], ζ = bufs[4], λ = bufs[5], σ²t = bufs[6], β = bufs[7], Σp = bufs[8], ρ = bufs[9], ν = bufs[10])
    catch
        ccall((:erm_farm_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), f[])
        rethrow()
    end
    M.farm = f[]                                            # the traces stay resident for checkConvergenceDevice (the farm's joint diagnostics)
    return M
end

"""
    sample!(MCMC; intercept=false, itemtype="2pl", cov2one, devices=nothing, waic=:off, ppc=0)

Same contract as the reference's `sample!`: runs `Cond.nIter * Cond.nChain` sweeps of the interleaved loop, fills
`MCMC.Post.{ra,rt,qr,logLike,mean}`, leaves the final state in `MCMC.Para`, returns `MCMC`.
`devices = 0:7` runs the `Cond.nChain` chains as independent chains, one per listed GPU (cycled), instead: `Post` has the same shapes,
chain `l` in slab `l`; `Post.mean` is the joint mean over iterations and chains.
`waic = :subject` or `:cell` also accumulates the pointwise log-likelihood on the device (`erm_set_pointwise`) for `getWaicDevice`; not with `devices`.
`ppc = true` or a thinning interval `>= 1` also replicates the data set on the device at every `ppc`-th post-burn-in sweep (`erm_set_predictive`) for `getPpcDevice`;
not with `devices`.
"""
function sample!(M::GibbsAMD; intercept = false, itemtype::Union{String} = "2pl",
                 cov2one = !(M isa GibbsRtIrtLatentQr || M isa GibbsRtIrtLatent), devices = nothing, waic::Symbol = :off, ppc::Union{Bool, Integer} = 0)
    if !(itemtype in ["1pl", "2pl"])
        error("Invalid input: the item type must be '1pl' or '2pl'.")
    end
    devices === nothing || waic == :off || error("WAIC is not available for a chain farm (devices)")
    thin = ppc === true ? 1 : Int(ppc)
    thin >= 0 || error("ppc must be false, true or a thinning interval >= 1")
    devices === nothing || thin == 0 || error("posterior predictive checks are not available for a chain farm (devices)")
    devices === nothing || return sampleFarm!(M, Bool(intercept), itemtype == "1pl", Bool(cov2one), collect(devices))
    C = M.Cond
    releaseFarm!(M)                                         # an earlier farm does not describe this run
    h = engine!(M, intercept, itemtype == "1pl", cov2one)
    check(ccall((:erm_reset_trace, LIB[]), Cint, (Ptr{Cvoid},), h))
    setPointwise!(M, waic)
    setPredictive!(M, thin)
    arrs = state_arrays(M.Para)
    GC.@preserve arrs begin
        st = ErmState(map(ptr, arrs)...)
        check(ccall((:erm_set_state, LIB[]), Cint, (Ptr{Cvoid}, Ref{ErmState}), h, st))
    end
    check(ccall((:erm_run, LIB[]), Cint, (Ptr{Cvoid}, Int64), h, C.nIter * C.nChain))

    trace(which) = begin
        w = ccall((:erm_trace_width, LIB[]), Int64, (Ptr{Cvoid}, Cint), h, which)
        out = Array{Float64}(undef, C.nIter, w, C.nChain)
        check(ccall((:erm_get_trace, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), h, which, out)); out
    end
    Post = M.Post
    Post.ra = trace(TRACE_RA)
    Post.logLike = trace(TRACE_LOGLIKE)
    modelid(M) != MODEL_MLIRT && (Post.rt = trace(TRACE_RT))
    Post.qr = trace(TRACE_QR)        # CrossQr: errors if vec(nu) per sweep exceeds erm_config.nu_trace_max_gb (then use erm_get_item_trace)

    N, J, F = C.nSubj, C.nItem, C.nFeat
    nb = modelid(M) == MODEL_MLIRT ? F + 1 : modelid(M) in (MODEL_RTIRT, MODEL_NULL) ? 2 * (F + 1) : modelid(M) in (MODEL_LATENTQR, MODEL_LATENT) ? F + 2 : 0
    nnu = modelid(M) == MODEL_LATENTQR ? N : modelid(M) == MODEL_CROSSQR ? N * J : 0
    bufs = (zeros(N), zeros(J), zeros(J), zeros(N), zeros(J), zeros(J), zeros(nb), zeros(4), zeros(J), zeros(nnu))
    GC.@preserve bufs begin
        check(ccall((:erm_get_mean, LIB[]), Cint, (Ptr{Cvoid}, Ref{ErmState}), h, ErmState(map(ptr, bufs)...)))
    end
    Post.mean = InputPara(θ = copy(bufs[1]), a = copy(bufs[2]), b = copy(bufs[3]), ζ = copy(bufs[4]), λ = copy(bufs[5]), σ²t = copy(bufs[6]),
                          β = copy(bufs[7]), Σp = copy(bufs[8]), ρ = copy(bufs[9]), ν = copy(bufs[10]))   # bufs are reused below
    GC.@preserve bufs begin
        check(ccall((:erm_get_state, LIB[]), Cint, (Ptr{Cvoid}, Ref{ErmState}), h, ErmState(map(ptr, bufs)...)))
    end
    P = M.Para
    P.θ, P.a, P.b = copy(bufs[1]), copy(bufs[2]), copy(bufs[3])
    if modelid(M) != MODEL_MLIRT
        P.ζ, P.λ, P.σ²t, P.Σp = copy(bufs[4]), copy(bufs[5]), copy(bufs[6]), reshape(copy(bufs[8]), 2, 2)
    end
    nb > 0 && (P.β = modelid(M) in (MODEL_RTIRT, MODEL_NULL) ? reshape(copy(bufs[7]), F + 1, 2) : copy(bufs[7]))
    modelid(M) in (MODEL_CROSSQR, MODEL_CROSS) && (P.ρ = copy(bufs[9]))
    modelid(M) == MODEL_CROSSQR && (P.ν = reshape(copy(bufs[10]), N, J))
    modelid(M) == MODEL_LATENTQR && (P.ν = copy(bufs[10]))
    return M
end

"""
    essRhat(MCMC, which) -> (ess, rhat)

Effective sample size and split R-hat of every column of `Post.ra` (`which = TRACE_RA`), `Post.rt` or `Post.qr`, computed on the device
from the resident traces (what `checkConvergence`, src/SimTools.jl:419-443, obtains from MCMCChains on the host).  Call after `sample!`.
"""
function essRhat(M::GibbsAMD, which::Integer)
    M.handle == C_NULL && error("run sample! first")
    w = ccall((:erm_trace_width, LIB[]), Int64, (Ptr{Cvoid}, Cint), M.handle, which)
    ess, rhat = zeros(w), zeros(w)
    check(ccall((:erm_get_diagnostics, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), M.handle, which, ess, rhat))
    return ess, rhat
end

"""
    rankEssRhat(MCMC, which) -> (essBulk, essTail, rhatRank)

Bulk-ESS, tail-ESS and rank-normalised split R-hat (Vehtari et al. 2021; what MCMCChains 6 reports from `ess_rhat`) of every column of `Post.ra`,
`Post.rt` or `Post.qr`, ranked and estimated on the device from the resident traces (`erm_get_rank_diagnostics`).  Call after `sample!`.
"""
function rankEssRhat(M::GibbsAMD, which::Integer)
    M.handle == C_NULL && error("run sample! first")
    w = ccall((:erm_trace_width, LIB[]), Int64, (Ptr{Cvoid}, Cint), M.handle, which)
    bulk, tail, rhat = zeros(w), zeros(w), zeros(w)
    check(ccall((:erm_get_rank_diagnostics, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.handle, which, bulk, tail, rhat))
    return bulk, tail, rhat
end

"""
    rankEssRhatDraws(x; precision=PREC_F64, device=0) -> (essBulk, essTail, rhatRank)

The same kernels on a host array `x[draw, column, chain]` of post-burn-in draws (`erm_debug_rank_diagnostics`): for traces that are not resident on one device.
"""
function rankEssRhatDraws(x::Array{Float64,3}; precision::Integer=1, device::Integer=0)
    nd, nc, nch = size(x)
    bulk, tail, rhat = zeros(nc), zeros(nc), zeros(nc)
    check(ccall((:erm_debug_rank_diagnostics, LIB[]), Cint, (Cint, Cint, Ptr{Float64}, Int64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, precision, x, nd, nc, nch, bulk, tail, rhat))
    return bulk, tail, rhat
end

"""
    getDicDevice(MCMC) -> (Dbar, Dhat, pD, DIC)

`getDic` (src/GibbsRtIrt.pl.jl:432-472, src/GibbsRtIrtCross.pl.jl:330-353, src/GibbsRtIrtLatent.pl.jl:342-365) from device-resident state
(`erm_get_dic`): D̄ over every recorded logLike row, D̂ from one evaluation pass at `Post.mean` on the device.  Call after `sample!`.
"""
function getDicDevice(M::GibbsAMD)
    M.handle == C_NULL && error("run sample! first")
    out = zeros(4)
    check(ccall((:erm_get_dic, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.handle, out))
    return (Dbar = out[1], Dhat = out[2], pD = out[3], DIC = out[4])
end

"""
    getWaicDevice(MCMC; pointwise = false) -> (elpd, pWaic, WAIC, se, lppd, nUnits, nRows, nHighVar[, lppd_u, p_u])

WAIC from the accumulators the engine keeps on the device (`erm_get_waic`; the reference offers DIC only).  Enable it before the run, while no trace row is
recorded: `setPointwise!(MCMC, :subject)` or `:cell` (`erm_set_pointwise`), then `sample!`.  The unit's log-likelihood is the data term of `getLogLikelihood*`
at each post-burn-in row (the conditional WAIC: the structural term is not part of it).  `pointwise = true` also fetches lppd_u and p_u
(`erm_get_pointwise`; subjects in order, cells as an nSubj x nItem matrix).
"""
function getWaicDevice(M::GibbsAMD; pointwise::Bool = false)
    M.handle == C_NULL && error("run sample! first")
    out = zeros(8)
    check(ccall((:erm_get_waic, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.handle, out))
    res = (elpd = out[1], pWaic = out[2], WAIC = out[3], se = out[4], lppd = out[5], nUnits = Int(out[6]), nRows = Int(out[7]), nHighVar = Int(out[8]))
    pointwise || return res
    U = ccall((:erm_pointwise_units, LIB[]), Int64, (Ptr{Cvoid},), M.handle)
    lppd_u, p_u = zeros(U), zeros(U)
    check(ccall((:erm_get_pointwise, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), M.handle, lppd_u, p_u))
    if U == M.Cond.nSubj * M.Cond.nItem && M.Cond.nItem > 1
        lppd_u, p_u = reshape(lppd_u, M.Cond.nSubj, M.Cond.nItem), reshape(p_u, M.Cond.nSubj, M.Cond.nItem)
    end
    return merge(res, (lppd_u = lppd_u, p_u = p_u))
end

"""
    getWaicMarginal(MCMC; nodes = 61, pointwise = false) -> (elpd, pWaic, WAIC, se, lppd, nUnits, nRows, nHighVar, nNodes, nCoarse[, lppd_u, p_u])

The marginal WAIC: every subject's θ and ζ integrated out (ζ in closed form, θ by a fixed rule of `nodes` equally spaced nodes), computed on the device after
`sample!` from the resident item-level trace and data set (`erm_get_marginal_waic`).  After `sample!(MCMC; devices=...)` the post-burn-in rows of all chains
enter as one table (`erm_farm_get_marginal_waic`).  Not for the two quantile models.  `nCoarse` counts the subjects whose posterior was too narrow for the rule
at some row: raise `nodes` until it is 0.
"""
function getWaicMarginal(M::GibbsAMD; nodes::Integer = 61, pointwise::Bool = false)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    out = zeros(10)
    lppd_u, p_u = pointwise ? (zeros(M.Cond.nSubj), zeros(M.Cond.nSubj)) : (Float64[], Float64[])
    pl, pp = pointwise ? (pointer(lppd_u), pointer(p_u)) : (Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL))
    GC.@preserve lppd_u p_u begin
        if farmed
            check(ccall((:erm_farm_get_marginal_waic, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, out, pl, pp))
        else
            check(ccall((:erm_get_marginal_waic, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, out, pl, pp))
        end
    end
    res = (elpd = out[1], pWaic = out[2], WAIC = out[3], se = out[4], lppd = out[5], nUnits = Int(out[6]), nRows = Int(out[7]), nHighVar = Int(out[8]),
           nNodes = Int(out[9]), nCoarse = Int(out[10]))
    return pointwise ? merge(res, (lppd_u = lppd_u, p_u = p_u)) : res
end

"""
    marginalLogLik(model, Y, logT, X, rows; nodes = 61, device = 0) -> l

The same kernel on caller-supplied data (`Y` UInt8 nSubj x nItem, `logT`, `X` nSubj x nFeat) and item-trace rows (`rows` is item_trace_width x nRows: one row of
`erm_get_item_trace` per column): `l[i, s]`, the marginal log-likelihood of subject i at row s (`erm_marginal_loglik`).  Scores new respondents against a saved
posterior.
"""
function marginalLogLik(model::Integer, Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}; nodes::Integer = 61, device::Integer = 0)
    N, J = size(Y)
    R = size(rows, 2)
    l = zeros(N, R)
    check(ccall((:erm_marginal_loglik, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, model, N, J, size(X, 2), Y, logT, X, rows, R, nodes, l, C_NULL, C_NULL, C_NULL))
    return l
end

# out12 and pw as erm_get_marginal_loo fills them (pw column-major [nSubj][4], the ERM_LOO_* columns) -> a named tuple
function looTuple(out::Vector{Float64}, pw::Matrix{Float64})
    res = (elpd = out[1], pLoo = out[2], LOOIC = out[3], se = out[4], lppd = out[5], nUnits = Int(out[6]), nRows = Int(out[7]), nBadK = Int(out[8]),
           nHighK = Int(out[9]), tailLen = Int(out[10]), nNodes = Int(out[11]), nCoarse = Int(out[12]))
    return isempty(pw) ? res : merge(res, (elpd_u = pw[:, 1], p_u = pw[:, 2], khat = pw[:, 3], nEff = pw[:, 4]))
end

"""
    getLooMarginal(MCMC; nodes = 61, pointwise = false) -> (elpd, pLoo, LOOIC, se, lppd, nUnits, nRows, nBadK, nHighK, tailLen, nNodes, nCoarse[, elpd_u, p_u, khat, nEff])

The marginal PSIS-LOO: Pareto-smoothed importance-sampling leave-one-subject-out on the marginal log-likelihoods of `getWaicMarginal`, computed on the device after
`sample!` (`erm_get_marginal_loo`; after `sample!(MCMC; devices=...)` over the rows of all chains, `erm_farm_get_marginal_loo`).  Needs 25 .. 8192 post-burn-in rows.
`khat` is the Pareto shape of a subject's importance ratios: above 0.7 (`nBadK`; `nHighK` counts those above min(1 - 1 / log10(nRows), 0.7)) the posterior would
move if the subject were left out -- an aberrant or highly influential respondent -- and `elpd_u` is optimistic; `Inf`: the tail could not be fitted.  Not for the
two quantile models.
"""
function getLooMarginal(M::GibbsAMD; nodes::Integer = 61, pointwise::Bool = false)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    out = zeros(12)
    pw = pointwise ? zeros(M.Cond.nSubj, 4) : zeros(0, 4)
    pp = pointwise ? pointer(pw) : Ptr{Float64}(C_NULL)
    GC.@preserve pw begin
        if farmed
            check(ccall((:erm_farm_get_marginal_loo, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, out, pp))
        else
            check(ccall((:erm_get_marginal_loo, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, out, pp))
        end
    end
    return looTuple(out, pw)
end

"""
    getWaicMarginalQr(MCMC; nodes = 61, pointwise = false) -> the named tuple of `getWaicMarginal`

The marginal WAIC of `GibbsRtIrtLatentQr` (= `GibbsRtIrtQuantile`): every subject's θ, ζ and quantile weight ν integrated out, at the sampler's `qRt`
(`erm_get_quantile_marginal_waic`; after `sample!(MCMC; devices=...)` `erm_farm_get_quantile_marginal_waic`).  With ν gone ζ given θ is asymmetric Laplace, and
its integral against the Gaussian response times is two normal-CDF terms.  The unit is the one of `getWaicMarginal`, so a `GibbsRtIrtLatent` fit and a
`GibbsRtIrtLatentQr` fit of the same data -- or two levels `qRt` -- can be compared subject by subject.  Not for `GibbsRtIrtCrossQr`.
"""
function getWaicMarginalQr(M::GibbsAMD; nodes::Integer = 61, pointwise::Bool = false)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    out = zeros(10)
    lppd_u, p_u = pointwise ? (zeros(M.Cond.nSubj), zeros(M.Cond.nSubj)) : (Float64[], Float64[])
    pl, pp = pointwise ? (pointer(lppd_u), pointer(p_u)) : (Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL))
    GC.@preserve lppd_u p_u begin
        if farmed
            check(ccall((:erm_farm_get_quantile_marginal_waic, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, out, pl, pp))
        else
            check(ccall((:erm_get_quantile_marginal_waic, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, out, pl, pp))
        end
    end
    res = (elpd = out[1], pWaic = out[2], WAIC = out[3], se = out[4], lppd = out[5], nUnits = Int(out[6]), nRows = Int(out[7]), nHighVar = Int(out[8]),
           nNodes = Int(out[9]), nCoarse = Int(out[10]))
    return pointwise ? merge(res, (lppd_u = lppd_u, p_u = p_u)) : res
end

"""
    getLooMarginalQr(MCMC; nodes = 61, pointwise = false) -> the named tuple of `getLooMarginal`

The marginal PSIS-LOO of `GibbsRtIrtLatentQr` on the marginal log-likelihoods of `getWaicMarginalQr` (`erm_get_quantile_marginal_loo`,
`erm_farm_get_quantile_marginal_loo`).  Needs 25 .. 8192 post-burn-in rows.
"""
function getLooMarginalQr(M::GibbsAMD; nodes::Integer = 61, pointwise::Bool = false)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    out = zeros(12)
    pw = pointwise ? zeros(M.Cond.nSubj, 4) : zeros(0, 4)
    pp = pointwise ? pointer(pw) : Ptr{Float64}(C_NULL)
    GC.@preserve pw begin
        if farmed
            check(ccall((:erm_farm_get_quantile_marginal_loo, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, out, pp))
        else
            check(ccall((:erm_get_quantile_marginal_loo, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, out, pp))
        end
    end
    return looTuple(out, pw)
end

"""
    quantileMarginalLogLik(Y, logT, X, rows, qRt; nodes = 61, device = 0) -> l

`marginalLogLik` for `GibbsRtIrtLatentQr` rows (Latent's layout) at the quantile level `qRt`, ν integrated out (`erm_quantile_marginal_loglik`).
"""
function quantileMarginalLogLik(Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}, qRt::Real; nodes::Integer = 61, device::Integer = 0)
    N, J = size(Y)
    R = size(rows, 2)
    l = zeros(N, R)
    check(ccall((:erm_quantile_marginal_loglik, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                device, MODEL_LATENTQR, N, J, size(X, 2), Y, logT, X, rows, R, qRt, nodes, l, C_NULL, C_NULL, C_NULL))
    return l
end

"""
    psisLoo(l; device = 0, weights = false) -> the named tuple of `getLooMarginal(...; pointwise = true)`[, lw]

The same kernel on a saved table `l[i, s]` of pointwise log-likelihoods (unit i, row s; what `marginalLogLik` returns -- a conditional table serves as well), 25 .. 8192
rows (`erm_psis_loo`).  `weights = true` adds `lw[i, s]`, the smoothed, normalised log-weights.
"""
function psisLoo(l::Matrix{Float64}; device::Integer = 0, weights::Bool = false)
    N, S = size(l)
    out, pw = zeros(12), zeros(N, 4)
    lw = weights ? zeros(N, S) : zeros(0, 0)
    GC.@preserve lw begin
        check(ccall((:erm_psis_loo, LIB[]), Cint, (Cint, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    device, l, N, S, out, pw, weights ? pointer(lw) : Ptr{Float64}(C_NULL)))
    end
    res = looTuple(out, pw)
    return weights ? merge(res, (lw = lw,)) : res
end

# score as erm_get_scores fills it (column-major [nSubj][7], the ERM_SCORE_* columns) and out4 -> a named tuple with the EAP reliabilities
function scoresTuple(score::Matrix{Float64}, out::Vector{Float64})
    mean(v) = sum(v) / length(v)
    rel(m, sd) = any(isnan, m) ? NaN : (b = mean((m .- mean(m)) .^ 2); b / (b + mean(sd .^ 2)))
    return (theta = score[:, 1], thetaSd = score[:, 2], zeta = score[:, 3], zetaSd = score[:, 4], cov = score[:, 5], rowEss = score[:, 6], coarse = score[:, 7] .!= 0.0,
            nRows = Int(out[2]), nNodes = Int(out[3]), nCoarse = Int(out[4]), relTheta = rel(score[:, 1], score[:, 2]), relZeta = rel(score[:, 3], score[:, 4]))
end

"""
    getScores(MCMC; nodes = 61) -> (theta, thetaSd, zeta, zetaSd, cov, rowEss, coarse, nRows, nNodes, nCoarse, relTheta, relZeta)

Scores of the subjects of the last `sample!`: the posterior mean and standard deviation of every θ_i and ζ_i and their covariance, computed on the device from the
resident item-level trace and data set in either trace mode (`erm_get_scores`; after `sample!(MCMC; devices=...)` over the rows of all chains,
`erm_farm_get_scores`), with the EAP reliabilities.  Posterior under the population law of `getWaicMarginal`: for the response-time models θ borrows strength from
the response times, so the scores differ from `Post.mean` by design; for GibbsMlIrt the two agree.  ζ, its sd and the covariance are NaN for GibbsMlIrt.  Not for
the two quantile models.
"""
function getScores(M::GibbsAMD; nodes::Integer = 61)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    score, out = zeros(M.Cond.nSubj, 7), zeros(4)
    if farmed
        check(ccall((:erm_farm_get_scores, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, score, out))
    else
        check(ccall((:erm_get_scores, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, score, out))
    end
    return scoresTuple(score, out)
end

"""
    scoreRespondents(model, Y, logT, X, rows; nodes = 61, weighting = :equal, device = 0, obs = nothing)

`getScores` for caller-supplied respondents (`Y` UInt8 nSubj x nItem, `logT`, `X` nSubj x nFeat) against saved item-trace rows (`rows` is item_trace_width x nRows,
as `marginalLogLik` takes them), on the device (`erm_score`).  `weighting = :equal`: every row counts once, the usual operational scoring; `:likelihood`: row s
counts exp(l_s), the posterior of a new respondent given their own data and the saved item posterior.
`obs` (UInt8 nSubj x nItem, 1 = the cell was administered): respondents who did not see every item (`erm_score_masked`) -- every sum over the items runs over the
observed cells, `Y` and `logT` at the others are never read; the result then also has `nObs`, the observed cells per respondent.
"""
function scoreRespondents(model::Integer, Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}; nodes::Integer = 61,
                          weighting::Symbol = :equal, device::Integer = 0, obs::Union{Nothing,Matrix{UInt8}} = nothing)
    N, J = size(Y)
    w = weighting == :equal ? 0 : weighting == :likelihood ? 1 : error("weighting must be :equal or :likelihood")
    score, out = zeros(N, 7), zeros(4)
    if obs === nothing
        check(ccall((:erm_score, LIB[]), Cint,
                    (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                    device, model, N, J, size(X, 2), Y, logT, X, rows, size(rows, 2), nodes, w, score, out))
        return scoresTuple(score, out)
    end
    size(obs) == (N, J) || error("obs does not match Y")
    nObs = zeros(Int32, N)
    check(ccall((:erm_score_masked, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}),
                device, model, N, J, size(X, 2), Y, logT, X, obs, rows, size(rows, 2), nodes, w, score, out, nObs))
    return merge(scoresTuple(score, out), (nObs = nObs,))
end

# fit as erm_get_person_fit fills it (column-major [nSubj][6], the ERM_FIT_* columns) and out4 -> a named tuple
fitTuple(fit::Matrix{Float64}, out::Vector{Float64}, nObs = nothing) =
    (lz = fit[:, 1], pResp = fit[:, 2], ltz = fit[:, 3], pTime = fit[:, 4], rowEss = fit[:, 5], coarse = fit[:, 6] .!= 0.0,
     nRows = Int(out[2]), nNodes = Int(out[3]), nCoarse = Int(out[4]), nObs = nObs)

"""
    getPersonFit(MCMC; nodes = 61) -> (lz, pResp, ltz, pTime, rowEss, coarse, nRows, nNodes, nCoarse, nObs)

Person fit of the subjects of the last `sample!`: whether each respondent's responses and response times are probable under the model for that person, computed on
the device from the resident item-level trace and data set in either trace mode (`erm_get_person_fit`; after `sample!(MCMC; devices=...)` over the rows of all
chains, `erm_farm_get_person_fit`).  `lz` is the standardised log-likelihood of the responses averaged over the posterior of θ (negative: misfit) and `pResp` its
posterior predictive p-value under the normal approximation; `ltz` is the Wilson-Hilferty z of the response-time quadratic form (positive: misfit) and `pTime` its
exact χ² posterior predictive p-value; small p-values mean misfit.  `ltz` and `pTime` are NaN for GibbsMlIrt.  Not for the two quantile models.
"""
function getPersonFit(M::GibbsAMD; nodes::Integer = 61)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    fit, out = zeros(M.Cond.nSubj, 6), zeros(4)
    if farmed
        check(ccall((:erm_farm_get_person_fit, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, fit, out))
    else
        check(ccall((:erm_get_person_fit, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, fit, out))
    end
    return fitTuple(fit, out)
end

"""
    personFit(model, Y, logT, X, rows; nodes = 61, weighting = :equal, device = 0, obs = nothing)

`getPersonFit` for caller-supplied respondents against saved item-trace rows, on the device (`erm_person_fit`); the arguments are `scoreRespondents`'.
`obs` (UInt8 nSubj x nItem, 1 = the cell was administered): respondents who did not see every item (`erm_person_fit_masked`) -- every sum runs over the observed
cells and the χ² has n_i degrees of freedom; a respondent without an observed cell has NaN in the four statistics; the result then has `nObs`.
"""
function personFit(model::Integer, Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}; nodes::Integer = 61,
                   weighting::Symbol = :equal, device::Integer = 0, obs::Union{Nothing,Matrix{UInt8}} = nothing)
    N, J = size(Y)
    w = weighting == :equal ? 0 : weighting == :likelihood ? 1 : error("weighting must be :equal or :likelihood")
    fit, out = zeros(N, 6), zeros(4)
    if obs === nothing
        check(ccall((:erm_person_fit, LIB[]), Cint,
                    (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                    device, model, N, J, size(X, 2), Y, logT, X, rows, size(rows, 2), nodes, w, fit, out))
        return fitTuple(fit, out)
    end
    size(obs) == (N, J) || error("obs does not match Y")
    nObs = zeros(Int32, N)
    check(ccall((:erm_person_fit_masked, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}),
                device, model, N, J, size(X, 2), Y, logT, X, obs, rows, size(rows, 2), nodes, w, fit, out, nObs))
    return fitTuple(fit, out, nObs)
end

# fit as erm_get_item_fit fills it (column-major [nItem][6], the ERM_IFIT_* columns) and out4 -> a named tuple
itemFitTuple(fit::Matrix{Float64}, out::Vector{Float64}) =
    (infit = fit[:, 1], outfit = fit[:, 2], respZ = fit[:, 3], rtMsq = fit[:, 4], rtZ = fit[:, 5], nObs = Int.(fit[:, 6]),
     nSubj = Int(out[1]), nRows = Int(out[2]), nNodes = Int(out[3]), nCoarse = Int(out[4]))

"""
    getItemFit(MCMC; nodes = 61) -> (infit, outfit, respZ, rtMsq, rtZ, nObs, nSubj, nRows, nNodes, nCoarse)

Item fit of the last `sample!`: per item the infit and outfit mean squares of the response residuals, the signed response residual `respZ` (negative: harder than
calibrated), the mean square `rtMsq` of the leave-one-item-out response-time residual and its signed sum `rtZ` (positive: slower than calibrated), computed on the
device from the resident item-level trace and data set (`erm_get_item_fit`; after `sample!(MCMC; devices=...)`, `erm_farm_get_item_fit`).  The two time columns are
NaN for GibbsMlIrt.  Not for the two quantile models.  A misfit that a free a_j or σ²t_j absorbs does not show on the calibration sample: check a second sample
with `itemFit`.
"""
function getItemFit(M::GibbsAMD; nodes::Integer = 61)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    fit, out = zeros(M.Cond.nItem, 6), zeros(4)
    if farmed
        check(ccall((:erm_farm_get_item_fit, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.farm, nodes, fit, out))
    else
        check(ccall((:erm_get_item_fit, LIB[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), M.handle, nodes, fit, out))
    end
    return itemFitTuple(fit, out)
end

"""
    itemFit(model, Y, logT, X, rows; nodes = 61, device = 0, obs = nothing)

`getItemFit` for a caller-supplied sample against saved item-trace rows, on the device (`erm_item_fit`): the drift check of a new sample against a saved
calibration.  The arguments are `scoreRespondents`' without the weighting.  `obs` (UInt8 nSubj x nItem, 1 = the cell was administered): an item's sums run over
the respondents that saw it, `nObs` counts them, an item nobody saw has NaN in the five statistics.
"""
function itemFit(model::Integer, Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}; nodes::Integer = 61, device::Integer = 0,
                 obs::Union{Nothing,Matrix{UInt8}} = nothing)
    N, J = size(Y)
    obs === nothing || size(obs) == (N, J) || error("obs does not match Y")
    fit, out = zeros(J, 6), zeros(4)
    check(ccall((:erm_item_fit, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Float64}),
                device, model, N, J, size(X, 2), Y, logT, X, obs === nothing ? C_NULL : obs, rows, size(rows, 2), nodes, fit, out))
    return itemFitTuple(fit, out)
end

# pv as erm_get_plausible_values fills it (column-major [nSubj][K][2]), node [nSubj][K], coarse [nSubj] and out4 -> a named tuple
pvTuple(pv::Array{Float64,3}, node::Matrix{Int32}, coarse::Vector{Int32}, out::Vector{Float64}, seed::UInt64) =
    (theta = pv[:, :, 1], zeta = pv[:, :, 2], node = node, coarse = coarse .!= 0, nRows = Int(out[2]), nNodes = Int(out[3]), nCoarse = Int(out[4]), seed = seed)

"""
    getPlausibleValues(MCMC; K = 5, seed = 20191, nodes = 61) -> (theta, zeta, node, coarse, nRows, nNodes, nCoarse, seed)

`K` plausible values per subject of the last `sample!`: draws of (θ_i, ζ_i) from each subject's posterior given the resident item-level trace, computed on the device in
either trace mode (`erm_get_plausible_values`; after `sample!(MCMC; devices=...)` over the rows of all chains, `erm_farm_get_plausible_values`).  `theta` and `zeta` are
nSubj x K (ζ is NaN for GibbsMlIrt): column k is one imputed data set.  Draws from the posterior `getScores` summarises; the same (K, seed, nodes) gives the same
draws.  Not for the two quantile models.
"""
function getPlausibleValues(M::GibbsAMD; K::Integer = 5, seed::Integer = 20191, nodes::Integer = 61)
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    1 <= K <= 4096 || error("K must be in 1 .. 4096")
    N = M.Cond.nSubj
    pv, node, coarse, out = zeros(N, K, 2), zeros(Int32, N, K), zeros(Int32, N), zeros(4)
    if farmed
        check(ccall((:erm_farm_get_plausible_values, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                    M.farm, nodes, K, seed, pv, node, coarse, out))
    else
        check(ccall((:erm_get_plausible_values, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                    M.handle, nodes, K, seed, pv, node, coarse, out))
    end
    return pvTuple(pv, node, coarse, out, UInt64(seed))
end

"""
    drawPlausibleValues(model, Y, logT, X, rows; K = 5, seed = 20191, nodes = 61, device = 0, obs = nothing)

`getPlausibleValues` for caller-supplied respondents (`Y` UInt8 nSubj x nItem, `logT`, `X` nSubj x nFeat) against saved item-trace rows (`rows` is
item_trace_width x nRows, as `marginalLogLik` takes them), on the device (`erm_plausible_values`); every row counts once.
`obs` (UInt8 nSubj x nItem, 1 = the cell was administered): respondents who did not see every item (`erm_plausible_values_masked`), as `scoreRespondents` takes
it; the result then also has `nObs`.
"""
function drawPlausibleValues(model::Integer, Y::Matrix{UInt8}, logT::Matrix{Float64}, X::Matrix{Float64}, rows::Matrix{Float64}; K::Integer = 5, seed::Integer = 20191,
                             nodes::Integer = 61, device::Integer = 0, obs::Union{Nothing,Matrix{UInt8}} = nothing)
    N, J = size(Y)
    1 <= K <= 4096 || error("K must be in 1 .. 4096")
    pv, node, coarse, out = zeros(N, K, 2), zeros(Int32, N, K), zeros(Int32, N), zeros(4)
    if obs === nothing
        check(ccall((:erm_plausible_values, LIB[]), Cint,
                    (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, UInt64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Float64}),
                    device, model, N, J, size(X, 2), Y, logT, X, rows, size(rows, 2), nodes, K, seed, pv, node, coarse, out))
        return pvTuple(pv, node, coarse, out, UInt64(seed))
    end
    size(obs) == (N, J) || error("obs does not match Y")
    nObs = zeros(Int32, N)
    check(ccall((:erm_plausible_values_masked, LIB[]), Cint,
                (Cint, Cint, Int64, Int32, Int32, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Int64, Int32, Int32, UInt64, Ptr{Float64}, Ptr{Int32},
                 Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                device, model, N, J, size(X, 2), Y, logT, X, obs, rows, size(rows, 2), nodes, K, seed, pv, node, coarse, out, nObs))
    return merge(pvTuple(pv, node, coarse, out, UInt64(seed)), (nObs = nObs,))
end

"""
    observedMask(Y, logT) -> Matrix{UInt8}

The observed mask of a data set whose missing cells are marked in the data: 1 where `Y` is 0 or 1 and `logT` is finite (`logT = nothing`, GibbsMlIrt: `Y` alone).
"""
observedMask(Y::AbstractMatrix, logT::Union{Nothing,AbstractMatrix} = nothing) =
    UInt8.(((Y .== 0) .| (Y .== 1)) .& (logT === nothing ? trues(size(Y)) : isfinite.(logT)))

"""
    setPointwise!(MCMC, unit)   # unit = :off | :subject | :cell

`erm_set_pointwise`: allowed only while no trace row is recorded (a fresh engine or after the trace was reset).
"""
function setPointwise!(M::GibbsAMD, unit::Symbol)
    M.handle == C_NULL && error("the engine does not exist yet")
    code = unit == :off ? 0 : unit == :subject ? 1 : unit == :cell ? 2 : error("unit must be :off, :subject or :cell")
    check(ccall((:erm_set_pointwise, LIB[]), Cint, (Ptr{Cvoid}, Cint), M.handle, code))
    return M
end

"""
    setPredictive!(MCMC, thin)   # thin = 0: off; thin >= 1: every thin-th post-burn-in sweep is replicated

`erm_set_predictive`: allowed only while no trace row is recorded (a fresh engine or after the trace was reset).
"""
function setPredictive!(M::GibbsAMD, thin::Integer)
    M.handle == C_NULL && error("the engine does not exist yet")
    check(ccall((:erm_set_predictive, LIB[]), Cint, (Ptr{Cvoid}, Cint, Int32), M.handle, thin > 0 ? 1 : 0, max(thin, 1)))
    return M
end

"""
    getPpcDevice(MCMC) -> (R, item, subj, total)

Posterior predictive checks from the accumulators the engine keeps on the device (`erm_get_predictive`; the reference has no counterpart).  Enable them before
the run: `sample!(MCMC; ppc = true)` (or `setPredictive!`).  `R` = the number of replicated data sets (`erm_predictive_reps`); `item` is nItem x 4 x 3, `subj`
nSubj x 4 x 2, `total` 4 x 2: unit x {n_ge, n_gt, mean_obs, mean_rep} x component (RA: response deviance, RT: response-time chi^2 -- NaN for GibbsMlIrt --,
SCORE: item score).  ppp = n_ge / R; mid-p = (n_gt + (n_ge - n_gt) / 2) / R.
"""
function getPpcDevice(M::GibbsAMD)
    M.handle == C_NULL && error("run sample! first")
    R = ccall((:erm_predictive_reps, LIB[]), Int64, (Ptr{Cvoid},), M.handle)
    item, subj, total = zeros(M.Cond.nItem, 4, 3), zeros(M.Cond.nSubj, 4, 2), zeros(4, 2)      # column-major: the C layout [component][quantity][unit]
    check(ccall((:erm_get_predictive, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), M.handle, item, subj, total))
    return (R = Int(R), item = item, subj = subj, total = total)
end

"""
    checkConvergenceDevice(MCMC; kind=:basic) -> (ess, rhat, essN, rhatN)
    checkConvergenceDevice(MCMC; kind=:rank)  -> (ess, essTail, rhat, essN, essTailN, rhatN)

`checkConvergence` (src/SimTools.jl:419-443) with the ESS / R-hat of every column computed AND counted on the device (`erm_get_convergence`).
`kind=:rank` counts the rank-normalised diagnostics instead (`erm_get_rank_convergence`): `ess` by bulk-ESS, `essTail` by tail-ESS, `rhat` by rank R-hat.
After `sample!(MCMC; devices=...)` the counts are the chain farm's: every estimator over the `nChain` independent chains jointly (`erm_farm_get_convergence` /
`erm_farm_get_rank_convergence`), which is where R-hat sees the variance between chains.  The sampler keeps that farm, with its resident traces, until its next
`sample!` for this purpose; nothing is computed before the call.
"""
function checkConvergenceDevice(M::GibbsAMD; kind::Symbol=:basic)
    kind in (:basic, :rank) || error("kind must be :basic or :rank")
    farmed = M.farm != C_NULL
    farmed || M.handle != C_NULL || error("run sample! first")
    n = kind == :rank ? 6 : 4
    tot = zeros(Int64, n)
    for which in (TRACE_RA, TRACE_RT, TRACE_QR)
        which == TRACE_RT && M isa GibbsMlIrt && continue
        c = zeros(Int64, n)
        if farmed && kind == :rank
            check(ccall((:erm_farm_get_rank_convergence, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}), M.farm, which, c))
        elseif farmed
            check(ccall((:erm_farm_get_convergence, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}), M.farm, which, c))
        elseif kind == :rank
            check(ccall((:erm_get_rank_convergence, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}), M.handle, which, c))
        else
            check(ccall((:erm_get_convergence, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}), M.handle, which, c))
        end
        tot .+= c
    end
    kind == :rank && return (ess = 100 * tot[2] / max(tot[1], 1), essTail = 100 * tot[4] / max(tot[3], 1), rhat = 100 * tot[6] / max(tot[5], 1),
                             essN = "$(tot[2]) / $(tot[1])", essTailN = "$(tot[4]) / $(tot[3])", rhatN = "$(tot[6]) / $(tot[5])")
    return (ess = 100 * tot[2] / max(tot[1], 1), rhat = 100 * tot[4] / max(tot[3], 1), essN = "$(tot[2]) / $(tot[1])", rhatN = "$(tot[4]) / $(tot[3])")
end

"""
    setSeed!(MCMC, seed)

A new seed for the chain's random streams (`erm_set_seed`): one sampler serves every replication of a `runSimulation` condition.
"""
function setSeed!(M::GibbsAMD, seed::Integer)
    M.seed = seed
    M.handle != C_NULL && check(ccall((:erm_set_seed, LIB[]), Cint, (Ptr{Cvoid}, UInt64), M.handle, UInt64(seed)))
    return M
end

"""
    simulateData!(MCMC, truePara; type="norm", seed=4321)

`setData*` on the device (src/SimTools.jl:117-368): draws X, theta, zeta, Y, logT from `truePara` straight into the engine's buffers;
`truePara.θ`, `truePara.ζ` receive the generated truth and `MCMC.Data` the data set.
"""
function simulateData!(M::GibbsAMD, truePara; type::String = "norm", seed = 4321)
    h = engine!(M, false, false, !(M isa GibbsRtIrtLatentQr || M isa GibbsRtIrtLatent); upload = false)
    arrs = state_arrays(truePara)
    GC.@preserve arrs begin
        check(ccall((:erm_simulate_data, LIB[]), Cint, (Ptr{Cvoid}, Ref{ErmState}, UInt64, Cint), h, ErmState(map(ptr, arrs)...), UInt64(seed),
                    type == "norm" ? 0 : type == "tail" ? 1 : 2))
    end
    C = M.Cond
    θ, ζ = zeros(C.nSubj), zeros(C.nSubj)
    check(ccall((:erm_get_truth, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h, θ, ζ))
    truePara.θ, truePara.ζ = θ, ζ
    Y = Array{UInt8}(undef, C.nSubj, C.nItem); logT = zeros(C.nSubj, C.nItem); X = zeros(C.nSubj, max(C.nFeat, 1))
    check(ccall((:erm_get_data, LIB[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}), h, Y, logT, X))
    M.Data = (Y = Y, κ = Y .- 0.5, T = exp.(logT), logT = logT, X = X[:, 1:C.nFeat])
    M.truePara = truePara
    return M
end

end # module

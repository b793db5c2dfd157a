"""Sampler objects and `sample!` for the MI355X engine -- host-side mirror of
/root/reference/src/GibbsRtIrt.pl.jl:35-472, src/GibbsRtIrtCross.pl.jl:55-353, src/GibbsRtIrtLatent.pl.jl:50-365.

Same struct names, fields (Cond, Data, truePara, Para, Post), constructor behaviour (always (re)initialises Para and
allocates Post), kwargs and error text as the reference.  `sample!` is spelled `sample_b` (PyJulia's convention for `!`)
and is also exported as `sample`.  All sampling happens in libertirt.so on the GPU; there is no CPU path here.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .base import InputPara, OutputDic, OutputLoo, OutputPpc, OutputPv, OutputScores, OutputWaic, SimConditions

_PREC = {"f32": _lib.PREC_F32, "f64": _lib.PREC_F64}
_TRACE = {"summary": _lib.TRACE_SUMMARY, "full": _lib.TRACE_FULL}


class _OutputPost:
    """OutputPostMlIrt / OutputPost / OutputPostCrossQr / OutputPostRtIrtLatentQr
    (src/GibbsRtIrt.pl.jl:35-71, src/GibbsRtIrtCross.pl.jl:55-69, src/GibbsRtIrtLatent.pl.jl:50-64).
    ra, rt, qr: (nIter, width, nChain); logLike: (nIter, 1, nChain); mean: InputPara with flat vectors."""

    def __init__(self):
        self.ra = np.zeros(0)
        self.rt = np.zeros(0)
        self.qr = np.zeros(0)
        self.logLike = np.zeros(0)
        self.mean = InputPara()


class _GibbsBase:
    _model = None
    _cov2one_default = True
    _has_intercept = True

    def __init__(self, Cond: SimConditions, *, Data=None, truePara=None, Para=None, Post=None,
                 seed=1234, device=0, precision="f64", trace="full", chain_id=0, shard=None, **engine_opts):
        self.Cond = Cond
        self.Data = Data
        self.truePara = truePara
        self.seed = int(seed)
        self.device = int(device)
        self.precision = precision
        self.trace = trace
        self.chain_id = int(chain_id)
        if not 0 <= self.chain_id <= 255:
            raise ValueError("chain_id must be in 0 .. 255 (the random streams carry eight bits of it)")
        # shard = (rank, count, nSubjTotal, rowBase, transport): this process holds subjects [rowBase, rowBase + Cond.nSubj) of ONE chain
        # spread over `count` devices (include/ertirt.h erm_set_shard*); transport = the 128-byte id of _lib.rccl_unique_id() (the
        # library's in-stream RCCL all-gather) or a callable exchange(send_ptr, recv_ptr, nbytes) such as parallel.TorchExchange.
        # Cond.nSubj, Data, Para.theta / zeta / nu and the subject blocks of Post then describe the local subjects only.
        self.shard = shard
        self.engine_opts = dict(engine_opts)
        self._engine = None
        self._engine_key = None
        self._data_on_device = False
        self.farm = None
        self.Para = None
        self.setInitialValues()          # constructors always overwrite Para (src/GibbsRtIrt.pl.jl:100-102)
        if shard is not None:
            self._shard_initial_values()
        self.Post = _OutputPost()

    def _shard_initial_values(self):
        """Initial values of a shard = the UNSHARDED sampler's initial values restricted to the local subjects: the whole-data-set
        state is generated (same seed on every rank, so item and structural entries agree bit for bit) and theta / zeta are cut."""
        import dataclasses
        rank, count, ntot, base, _ = self.shard
        local = self.Cond
        if not (0 <= base and base + local.nSubj <= ntot):
            raise ValueError("shard: local subjects must lie inside [0, nSubjTotal)")
        self.Cond = dataclasses.replace(local, nSubj=int(ntot))
        try:
            self.setInitialValues()
        finally:
            self.Cond = local
        for f in ("theta", "zeta"):
            v = getattr(self.Para, f)
            if np.size(v) == ntot:
                setattr(self.Para, f, np.ascontiguousarray(np.asarray(v)[base:base + local.nSubj]))

    @property
    def _traits(self):
        return _lib.MODEL_TRAITS[self._model]

    def setInitialValues(self):
        """The constructors' initial values (setInitialValues of src/GibbsRtIrt.pl.jl:84,122,159; src/GibbsRtIrtCross.pl.jl:85,123;
        src/GibbsRtIrtLatent.pl.jl:78,113), from the sampler's own stream.  The draws come in this order: theta, zeta if the model has response
        times, then beta or rho."""
        C, g, t = self.Cond, self._rng(), self._traits
        init = dict(theta=g.standard_normal(C.nSubj), a=np.ones(C.nItem), b=np.zeros(C.nItem))
        if t.rt:
            init.update(zeta=g.standard_normal(C.nSubj), lam=np.zeros(C.nItem), sig2t=np.ones(C.nItem), Sigp=np.eye(2))
        if t.beta in ("vec", "pair", "latent"):
            init["beta"] = g.standard_normal(_lib.beta_shape(self._model, C.nFeat))
        if t.rho:
            init["rho"] = g.standard_normal(C.nItem)
        self.Para = InputPara(**init)
        return self

    def _rng(self):
        return np.random.default_rng(np.random.SeedSequence([self.seed, self.chain_id, 0x1217]))

    def _state_for_engine(self):
        P = self.Para
        d = dict(theta=P.theta, a=P.a, b=P.b)
        if self._traits.rt:
            d.update(zeta=P.zeta, lambda_=P.lam, sig2t=P.sig2t, sigp=np.asarray(P.Sigp, dtype=np.float64).reshape(-1, order="F"))
        if P.beta.size:
            d["beta"] = np.asarray(P.beta, dtype=np.float64).reshape(-1, order="F")
        if P.rho.size:
            d["rho"] = P.rho
        if P.nu.size and self._traits.nu != "none":
            d["nu"] = np.asarray(P.nu, dtype=np.float64).reshape(-1, order="F")
        return d

    def _engine_for(self, intercept, onepl, cov2one, *, upload=True):
        key = (bool(intercept), bool(onepl), bool(cov2one))
        if self._engine is not None and self._engine_key == key:
            return self._engine
        resident = None
        if self._engine is not None:
            if not upload or self._data_on_device:
                resident = self._engine.get_data()     # the data set lives on the device only: carry it over to the new engine
            self._engine.close()
        C = self.Cond
        if self.Data is None and upload and resident is None:
            raise ValueError("Data is required")
        eng = _lib.Engine(model=self._model, n_item=C.nItem, n_subj=C.nSubj, n_feat=C.nFeat, n_iter=C.nIter, n_chain=C.nChain,
                          n_burnin=C.nBurnin, intercept=int(intercept), one_pl=int(onepl), cov2one=int(cov2one), q_rt=C.qRt,
                          seed=self.seed, chain_id=self.chain_id, device=self.device, precision=_PREC[self.precision],
                          trace_mode=_TRACE[self.trace], **self.engine_opts)
        self._engine, self._engine_key = eng, key
        if self.shard is not None:
            rank, count, ntot, base, transport = self.shard
            if callable(transport):
                eng.set_shard(rank, count, ntot, base, transport)
            else:
                eng.set_shard_rccl(rank, count, ntot, base, transport)
        if resident is not None:
            eng.set_data(*resident)
            return eng
        if not upload:
            return eng
        D = self.Data
        Y = np.asarray(D.Y)
        if Y.shape != (C.nSubj, C.nItem):
            raise ValueError(f"Data.Y must be {C.nSubj}x{C.nItem}, got {Y.shape}")
        logT = None
        if self._traits.rt:
            logT = np.asarray(D.logT, dtype=np.float64)
            if logT.shape != (C.nSubj, C.nItem):
                raise ValueError(f"Data.logT must be {C.nSubj}x{C.nItem}, got {logT.shape}")
        X = None
        if self._traits.sees_x and C.nFeat > 0:
            X = np.asarray(D.X, dtype=np.float64)
            if X.shape != (C.nSubj, C.nFeat):
                raise ValueError(f"Data.X must be {C.nSubj}x{C.nFeat}, got {X.shape}")
        eng.set_data(Y, logT, X)
        self._engine, self._engine_key = eng, key
        return eng

    def _fill_post(self, eng):
        C = self.Cond
        Post = self.Post
        full = self.trace == "full"
        Post.logLike = eng.trace(_lib.TRACE_LOGLIKE)
        if full:
            Post.ra = eng.trace(_lib.TRACE_RA)
            if self._traits.rt:
                Post.rt = eng.trace(_lib.TRACE_RT)
            try:
                Post.qr = eng.trace(_lib.TRACE_QR)
            except _lib.ErmError:
                if self._traits.nu != "cell":
                    raise
                # vec(nu) per sweep did not fit the device budget: Post.qr keeps [rho; vec(Sigp)] (the reference's first nItem+4 columns)
                it = eng.item_trace()
                Post.qr = np.asfortranarray(it[:, 4 * C.nItem:].reshape(C.nIter, C.nChain, -1).transpose(0, 2, 1))
        Post.item_trace = eng.item_trace()
        m = eng.get_mean()
        mean = InputPara(theta=m["theta"], a=m["a"], b=m["b"])
        if self._traits.rt:
            mean.zeta, mean.lam, mean.sig2t = m["zeta"], m["lambda_"], m["sig2t"]
            mean.Sigp = m["sigp"]
        if m["beta"] is not None:
            mean.beta = m["beta"]
        if self._traits.rho:
            mean.rho = m["rho"]
        if m["nu"] is not None:
            mean.nu = m["nu"]
        Post.mean = mean

    def _update_para(self, eng):
        s = eng.get_state()
        C = self.Cond
        P = self.Para
        t = self._traits
        P.theta, P.a, P.b = s["theta"], s["a"], s["b"]
        if t.rt:
            P.zeta, P.lam, P.sig2t = s["zeta"], s["lambda_"], s["sig2t"]
            P.Sigp = s["sigp"].reshape(2, 2, order="F")
        if s["beta"] is not None:
            P.beta = s["beta"].reshape(_lib.beta_shape(self._model, C.nFeat), order="F")
        if t.rho:
            P.rho = s["rho"]
        if t.nu == "cell":
            P.nu = s["nu"].reshape(C.nSubj, C.nItem, order="F")
        if t.nu == "subject":
            P.nu = s["nu"]

    def timing(self):
        return self._engine.timing() if self._engine is not None else None

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        if getattr(self, "farm", None) is not None:
            self.farm.close()
            self.farm = None


def simulateData(MCMC: _GibbsBase, truePara: InputPara, *, type="norm", seed=4321, pull=True, pull_truth=True, intercept=False, itemtype="2pl", cov2one=None):
    """setData* on the device (erm_simulate_data): generates X, theta, zeta, Y, logT from `truePara` straight into the engine's
    resident buffers -- no host generation, no upload.  truePara.theta / .zeta receive the generated truth (pull_truth=False leaves it on the
    device); with pull=True the data set is also copied to MCMC.Data (the host-side getLogLikelihood / getDicHost need it; getDic does not)."""
    from .base import InputData
    # (the engine is keyed by the sample! kwargs: give the ones the following sample! will use, or the data set is carried over through the host)
    eng = MCMC._engine_for(intercept, itemtype == "1pl", MCMC._cov2one_default if cov2one is None else cov2one, upload=False)
    noise = {"norm": 0, "tail": 1, "skew": 2}[type]
    truth = dict(a=truePara.a, b=truePara.b)
    if MCMC._traits.rt:
        truth.update(lambda_=truePara.lam, sig2t=truePara.sig2t if truePara.sig2t.size else np.ones(MCMC.Cond.nItem))
        if np.size(truePara.Sigp):
            truth["sigp"] = np.asarray(truePara.Sigp, dtype=np.float64).reshape(-1, order="F")
    if truePara.beta.size:
        truth["beta"] = np.asarray(truePara.beta, dtype=np.float64).reshape(-1, order="F")
    if truePara.rho.size:
        truth["rho"] = truePara.rho
    tz = eng.simulate_data(seed=seed, noise=noise, pull_truth=pull_truth, **truth)
    if pull_truth:
        truePara.theta, truePara.zeta = tz
    MCMC.truePara = truePara
    MCMC._data_on_device = True
    if pull:
        Y, logT, X = eng.get_data()
        MCMC.Data = InputData(Y=Y, T=np.exp(logT) if logT is not None else (), X=X if X is not None else ())
    return MCMC


def _sample_farm(MCMC: _GibbsBase, intercept, onepl, cov2one, devices):
    """sample! with Cond.nChain INDEPENDENT chains, chain l on GPU devices[l mod len(devices)] (erm_farm_*, include/ertirt.h): the chains
    run concurrently inside the library, Post.ra / rt / qr / logLike get chain l in slab l, and Post.mean is the joint mean over
    iterations and chains (src/GibbsRtIrt.pl.jl:327-343) reduced over the devices by one RCCL all-reduce.  Chain 0 starts from
    MCMC.Para (the constructor's setInitialValues); chain l > 0 from its own setInitialValues draw on random stream l."""
    import copy
    C = MCMC.Cond
    if MCMC.shard is not None:
        raise ValueError("a subject-sharded sampler cannot also farm chains")
    if MCMC.Data is None:
        raise ValueError("Data is required")
    devs = [int(devices[l % len(devices)]) for l in range(C.nChain)]
    farm = _lib.Farm(devs, model=MCMC._model, n_item=C.nItem, n_subj=C.nSubj, n_feat=C.nFeat, n_iter=C.nIter, n_chain=1, n_burnin=C.nBurnin,
                     intercept=int(intercept), one_pl=int(onepl), cov2one=int(cov2one), q_rt=C.qRt, seed=MCMC.seed, precision=_PREC[MCMC.precision],
                     trace_mode=_TRACE[MCMC.trace], **MCMC.engine_opts)
    D = MCMC.Data
    logT = np.asarray(D.logT, dtype=np.float64) if MCMC._traits.rt else None
    X = None
    if MCMC._traits.sees_x and C.nFeat > 0:
        X = np.asarray(D.X, dtype=np.float64)
    farm.set_data(np.asarray(D.Y), logT, X)
    for l in range(C.nChain):
        if l == 0:
            farm.set_state(0, **MCMC._state_for_engine())
        else:
            other = copy.copy(MCMC)
            other.chain_id = l
            other.setInitialValues()
            farm.set_state(l, **other._state_for_engine())
    farm.run(C.nIter)
    MCMC._fill_post(farm)
    MCMC._update_para(farm.engine(0))
    MCMC.farm = farm
    return MCMC


def sample_b(MCMC: _GibbsBase, *, intercept=False, itemtype="2pl", cov2one=None, devices=None, fill=True, waic=None, ppc=None):
    """sample!(MCMC; intercept, itemtype, cov2one) -- src/GibbsRtIrt.pl.jl:210,278; Cross :265; Latent :271.
    Runs Cond.nIter * Cond.nChain sweeps (the reference's interleaved `for m in 1:nIter, l in 1:nChain` loop over ONE
    shared Para), fills MCMC.Post, leaves the final state in MCMC.Para and returns MCMC.
    devices = [gpu ordinals]: the nChain chains become INDEPENDENT chains farmed over those GPUs instead (see _sample_farm).
    fill = False leaves Post and Para untouched: traces, running means and the final state stay on the device, where getDic,
    checkConvergence and MCMC._engine.get_mean(which) read them (runSimulation's replications cross the boundary with summaries only).
    waic = "subject" | "cell": the engine also accumulates the pointwise log-likelihood of every subject / cell over the post-burn-in sweeps (erm_set_pointwise;
    one more streaming pass per sweep, the chain itself is unchanged); getWaic reads it.  Not available with devices=.
    ppc = True | thin (an int >= 1): the engine also replicates the data set at every thin-th post-burn-in sweep and accumulates the posterior predictive checks of every
    item, subject and the whole fit (erm_set_predictive; the chain itself is unchanged); getPpc reads them.  Not available with devices=."""
    if ppc is not None and ppc is not False and (isinstance(ppc, (bool, np.bool_)) is False and (not isinstance(ppc, (int, np.integer)) or ppc < 1)):
        raise ValueError("ppc must be None, True or a thinning interval >= 1")
    ppc_thin = 0 if ppc is None or ppc is False else int(ppc)      # True -> 1
    if ppc_thin and (devices is not None or MCMC.shard is not None):
        raise ValueError("posterior predictive checks are not available for a chain farm (devices=) or a subject-sharded sampler: the accumulators of several devices are not merged")
    if waic not in _lib.POINTWISE_UNITS:
        raise ValueError("waic must be None, 'subject' or 'cell'")
    if waic is not None and (devices is not None or MCMC.shard is not None):
        raise ValueError("WAIC is not available for a chain farm (devices=) or a subject-sharded sampler: the accumulators of several devices are not merged")
    if itemtype not in ("1pl", "2pl"):
        raise ValueError("Invalid input: the item type must be '1pl' or '2pl'.")   # same text as :213,281
    if cov2one is None:
        cov2one = MCMC._cov2one_default
    if intercept and not MCMC._has_intercept:
        raise TypeError(f"sample! for {type(MCMC).__name__} has no `intercept` keyword")
    if devices is not None:
        return _sample_farm(MCMC, intercept, itemtype == "1pl", cov2one, list(devices))
    if MCMC.farm is not None:
        MCMC.farm.close()
        MCMC.farm = None
    eng = MCMC._engine_for(intercept, itemtype == "1pl", cov2one)
    eng.reset_trace()
    if waic is not None or eng.pointwise_units:
        eng.set_pointwise(waic)
    MCMC._waic_unit = waic
    if ppc_thin or eng.predictive_reps or getattr(MCMC, "_ppc_thin", 0):
        eng.set_predictive(ppc_thin > 0, max(ppc_thin, 1))
    MCMC._ppc_thin = ppc_thin
    eng.set_state(**MCMC._state_for_engine())
    eng.run(MCMC.Cond.nIter * MCMC.Cond.nChain)
    if fill:
        MCMC._fill_post(eng)
        MCMC._update_para(eng)
    return MCMC


sample = sample_b


class GibbsMlIrt(_GibbsBase):
    """src/GibbsRtIrt.pl.jl:76-106.  theta's prior variance is 1 (the reference never sets Para.Σp for this model:
    :85-91, :228; its likelihood uses Normal(mu, 1.) :201)."""
    _model = _lib.MODEL_MLIRT


class GibbsRtIrt(_GibbsBase):
    """src/GibbsRtIrt.pl.jl:114-146"""
    _model = _lib.MODEL_RTIRT


class GibbsRtIrtCrossQr(_GibbsBase):
    """src/GibbsRtIrtCross.pl.jl:115-147"""
    _model = _lib.MODEL_CROSSQR
    _has_intercept = False


class GibbsRtIrtLatentQr(_GibbsBase):
    """src/GibbsRtIrtLatent.pl.jl:105-137 (sample! default cov2one = false, :271)"""
    _model = _lib.MODEL_LATENTQR
    _cov2one_default = False


class GibbsRtIrtNull(_GibbsBase):
    """src/GibbsRtIrt.pl.jl:151-183: no latent regression (beta = 0 every sweep, :380), theta ~ N(0, Sigp11), zeta ~ N(0, 1)."""
    _model = _lib.MODEL_NULL
    _has_intercept = False


class GibbsRtIrtCross(_GibbsBase):
    """src/GibbsRtIrtCross.pl.jl:77-110: cross-relation rho without quantile weights."""
    _model = _lib.MODEL_CROSS
    _has_intercept = False


class GibbsRtIrtLatent(_GibbsBase):
    """src/GibbsRtIrtLatent.pl.jl:70-102 (sample! default cov2one = false, :168): zeta regressed on [1 X theta], beta drawn."""
    _model = _lib.MODEL_LATENT
    _cov2one_default = False


# README.md:22,95 names `GibbsRtIrtQuantile`; the export is commented out in the reference (src/ExtendedRtIrtModeling.jl:65) and
# the only live type with that API (X, beta, Sigp, qRt) is GibbsRtIrtLatentQr.
GibbsRtIrtQuantile = GibbsRtIrtLatentQr


# ------------------------------------------------------------------------------------------------------------------
# log-likelihoods at a parameter point and DIC (host-side post-processing, numpy fp64)
# ------------------------------------------------------------------------------------------------------------------
def _log1pexp(x):
    return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(-np.abs(x))))


def _norm_logpdf(x, mu, sd):
    return -0.5 * np.log(2 * np.pi) - np.log(sd) - 0.5 * ((x - mu) / sd) ** 2


def getLogLikelihood(MCMC: _GibbsBase, P: InputPara) -> float:
    """getLogLikelihoodMlIrt / RtIrt / RtIrtNull / RtIrtCross(Qr) / RtIrtLatent(Qr) evaluated at P
    (src/GibbsRtIrt.pl.jl:195-204,262-272,351-362; src/GibbsRtIrtCross.pl.jl:158-170,240-258; src/GibbsRtIrtLatent.pl.jl:151-162,243-264)."""
    C, D = MCMC.Cond, MCMC.Data
    Y = np.asarray(D.Y, dtype=np.float64)
    th, a, b = P.theta, P.a, P.b
    pr = a[None, :] * (th[:, None] - b[None, :])
    ll = np.sum(Y * pr - _log1pexp(pr))
    m = MCMC._model
    if m == _lib.MODEL_MLIRT:
        x = np.column_stack([np.ones(C.nSubj), D.X])
        return float(ll + np.sum(_norm_logpdf(th, x @ P.beta, 1.0)))
    q = C.qRt
    k1, k2 = (1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))
    logT = np.asarray(D.logT, dtype=np.float64)
    nu_lat = P.nu
    if m in (_lib.MODEL_NULL, _lib.MODEL_CROSS, _lib.MODEL_LATENT):
        k1, k2, nu_lat = 0.0, 1.0, 1.0            # no quantile weights
    if m == _lib.MODEL_CROSS:
        mut = P.lam[None, :] - P.zeta[:, None] - th[:, None] * P.rho[None, :]
        ll += np.sum(_norm_logpdf(logT, mut, np.sqrt(P.sig2t)[None, :]))
    elif m == _lib.MODEL_CROSSQR:
        e = np.asarray(P.nu).reshape(C.nSubj, C.nItem, order="F")
        mut = P.lam[None, :] - P.zeta[:, None] - th[:, None] * P.rho[None, :] + k1 * e
        ll += np.sum(_norm_logpdf(logT, mut, np.sqrt(P.sig2t[None, :] * (k2 * e))))
    else:
        ll += np.sum(_norm_logpdf(logT, P.lam[None, :] - P.zeta[:, None], np.sqrt(P.sig2t)[None, :]))
    S = np.asarray(P.Sigp, dtype=np.float64).reshape(2, 2, order="F")
    if m in (_lib.MODEL_RTIRT, _lib.MODEL_CROSSQR, _lib.MODEL_NULL, _lib.MODEL_CROSS):
        eta = np.column_stack([th, P.zeta])
        if m == _lib.MODEL_RTIRT:
            x = np.column_stack([np.ones(C.nSubj), D.X])
            eta = eta - x @ np.asarray(P.beta).reshape(C.nFeat + 1, 2, order="F")
        Si = np.linalg.inv(S)
        quad = np.einsum("ia,ab,ib->i", eta, Si, eta)
        ll += np.sum(-np.log(2 * np.pi) - 0.5 * np.log(np.linalg.det(S)) - 0.5 * quad)
    else:
        x = np.column_stack([np.ones(C.nSubj), D.X, th])
        ll += np.sum(_norm_logpdf(P.zeta, x @ P.beta + k1 * nu_lat, np.sqrt(S[1, 1] * k2 * nu_lat)))
    return float(ll)


def getDicHost(MCMC: _GibbsBase) -> OutputDic:
    """getDic evaluated with numpy on the host from MCMC.Data and MCMC.Post (the test twin of the device path below; needs the data set and
    Post.mean on the host)."""
    Dhat = -2.0 * getLogLikelihood(MCMC, MCMC.Post.mean)
    Dbar = -2.0 * float(np.mean(MCMC.Post.logLike))
    pD = Dbar - Dhat
    return OutputDic(pD=pD, DIC=Dbar + pD)


def getDic(MCMC: _GibbsBase) -> OutputDic:
    """src/GibbsRtIrt.pl.jl:432-458 (and Cross :329-353, Latent :341-365): D̂ = -2 logLik(Post.mean),
    D̄ = -2 mean(Post.logLike) over ALL iterations (burn-in included, as the reference does).  Computed by the engine from device-resident
    state (erm_get_dic / erm_farm_get_dic: the logLike rows, the running sums behind Post.mean and ONE evaluation pass over the resident data
    set): neither the data set nor an N-wide mean has to be on the host.  Call it after sample!, before the sampler is closed."""
    src = getattr(MCMC, "farm", None) or MCMC._engine
    if src is None:
        raise ValueError("run sample! first (getDic reads the engine's resident state)")
    d = src.dic()
    return OutputDic(pD=d["pD"], DIC=d["DIC"])


# ------------------------------------------------------------------------------------------------------------------
# WAIC.  Unit u = a subject or a cell; l_u^(s) = the unit's part of the DATA term of getLogLikelihood at the values of post-burn-in trace row s
# (the structural term -- theta, zeta given beta, Sigp -- is not part of it: the conditional WAIC, leave-one-unit-out given the subject's own parameters).
# ------------------------------------------------------------------------------------------------------------------
def getWaic(MCMC: _GibbsBase, pointwise=False) -> OutputWaic:
    """WAIC of the last sample!(...; waic="subject" | "cell"), from the accumulators the engine kept on the device (erm_get_waic: the per-unit finish and the
    totals are computed there).  pointwise=True also fetches lppd_u and p_u (erm_get_pointwise), which compareWaic needs."""
    if getattr(MCMC, "farm", None) is not None:
        raise ValueError("getWaic is not available for a sampler run through devices= (a chain farm keeps no WAIC accumulators)")
    eng, unit = MCMC._engine, getattr(MCMC, "_waic_unit", None)
    if eng is None or unit is None:
        raise ValueError("run sample!(...; waic='subject' or 'cell') first (getWaic reads the engine's resident accumulators)")
    w = eng.waic()
    out = OutputWaic(elpd=w["elpd"], pWaic=w["pWaic"], WAIC=w["WAIC"], se=w["se"], nHighVar=w["nHighVar"], lppd=w["lppd"], unit=unit, nUnits=w["nUnits"], nRows=w["nRows"])
    if pointwise:
        out.lppd_u, out.p_u = eng.pointwise()
    return out


def pointwiseLogLikHost(MCMC: _GibbsBase, unit) -> np.ndarray:
    """l_u^(s) for every post-burn-in row s (iteration >= nBurnin, every interleaved chain) and unit u, with numpy from MCMC.Data and the full Post traces:
    an (|S|, U) array; cells in column-major order of (nSubj, nItem)."""
    if unit not in ("subject", "cell"):
        raise ValueError("unit must be 'subject' or 'cell'")
    C, D, P, m = MCMC.Cond, MCMC.Data, MCMC.Post, MCMC._model
    N, J = C.nSubj, C.nItem
    if np.ndim(P.ra) != 3:
        raise ValueError("getWaicHost needs the full Post traces (trace='full' and fill=True)")
    Y = np.asarray(D.Y, dtype=np.float64)
    logT = None if m == _lib.MODEL_MLIRT else np.asarray(D.logT, dtype=np.float64)
    q = C.qRt
    k1, k2 = ((1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))) if m == _lib.MODEL_CROSSQR else (0.0, 1.0)
    if m == _lib.MODEL_CROSSQR and P.qr.shape[1] != J + 4 + N * J:
        raise ValueError("getWaicHost needs the per-sweep nu trace of GibbsRtIrtCrossQr in Post.qr")
    rows = [(it, l) for it in range(C.nBurnin, C.nIter) for l in range(C.nChain)]
    out = np.empty((len(rows), N * J if unit == "cell" else N))
    for s, (it, l) in enumerate(rows):
        ra = P.ra[it, :, l]
        th, a, b = ra[:N], ra[N:N + J], ra[N + J:N + 2 * J]
        eta = a[None, :] * (th[:, None] - b[None, :])
        ll = Y * eta - _log1pexp(eta)
        if m != _lib.MODEL_MLIRT:
            rt = P.rt[it, :, l]
            ze, lam, sg = rt[:N], rt[N:N + J], rt[N + J:N + 2 * J]
            mu = lam[None, :] - ze[:, None]
            var = np.broadcast_to(sg[None, :], (N, J))
            if m in (_lib.MODEL_CROSS, _lib.MODEL_CROSSQR):
                qr = P.qr[it, :, l]
                mu = mu - th[:, None] * qr[None, :J]
                if m == _lib.MODEL_CROSSQR:
                    nu = qr[J + 4:].reshape(N, J, order="F")
                    mu = mu + k1 * nu
                    var = sg[None, :] * (k2 * nu)
            ll = ll + _norm_logpdf(logT, mu, np.sqrt(var))
        out[s] = ll.reshape(-1, order="F") if unit == "cell" else ll.sum(axis=1)
    return out


def getWaicHost(MCMC: _GibbsBase, unit) -> OutputWaic:
    """getWaic evaluated with numpy on the host (the test twin of the device path): scipy's logsumexp and np.var(ddof=1) over pointwiseLogLikHost's rows."""
    from scipy.special import logsumexp
    L = pointwiseLogLikHost(MCMC, unit)
    S, U = L.shape
    if S < 2:
        raise ValueError("WAIC needs at least two post-burn-in rows")
    lppd_u = logsumexp(L, axis=0) - np.log(S)
    p_u = np.var(L, axis=0, ddof=1)
    el = lppd_u - p_u
    elpd = float(np.sum(el))
    se = 2.0 * float(np.sqrt(U * np.var(el, ddof=1))) if U > 1 else 0.0
    if unit == "cell":
        sh = (MCMC.Cond.nSubj, MCMC.Cond.nItem)
        lppd_u, p_u = lppd_u.reshape(sh, order="F"), p_u.reshape(sh, order="F")
    return OutputWaic(elpd=elpd, pWaic=float(np.sum(p_u)), WAIC=-2.0 * elpd, se=se, nHighVar=int(np.sum(p_u > 0.4)), lppd=float(np.sum(lppd_u)), unit=unit, nUnits=U,
                      nRows=S, lppd_u=lppd_u, p_u=p_u)


def compareWaic(A, B) -> dict:
    """Two fits of the SAME data compared unit by unit: elpd_diff = sum_u (elpd_u^A - elpd_u^B) (positive: A predicts better) and its standard error
    se_diff = sqrt(U Var_u(elpd_u^A - elpd_u^B)).  A, B: samplers (getWaic(pointwise=True) is called) or OutputWaic objects that carry the pointwise vectors -- or
    two OutputLoo objects (getLooMarginal(pointwise=True)): the same paired difference on the PSIS-LOO elpd_u (compareLoo)."""
    if isinstance(A, OutputLoo) or isinstance(B, OutputLoo):
        if not (isinstance(A, OutputLoo) and isinstance(B, OutputLoo)):
            raise ValueError("compareWaic: an OutputLoo can only be compared with another OutputLoo")
        wa, wb = A, B
    else:
        wa = A if isinstance(A, OutputWaic) else getWaic(A, pointwise=True)
        wb = B if isinstance(B, OutputWaic) else getWaic(B, pointwise=True)
    if wa.lppd_u is None or wb.lppd_u is None:
        raise ValueError("compareWaic needs the pointwise values (getWaic(..., pointwise=True))")
    if wa.unit != wb.unit:
        raise ValueError(f"compareWaic: the fits use different units ({wa.unit!r} and {wb.unit!r})")
    if np.shape(wa.lppd_u) != np.shape(wb.lppd_u):
        raise ValueError(f"compareWaic: the fits have different numbers of units ({np.size(wa.lppd_u)} and {np.size(wb.lppd_u)})")
    d = np.ravel(wa.elpd_u) - np.ravel(wb.elpd_u)
    U = d.size
    return dict(elpd_diff=float(np.sum(d)), se_diff=float(np.sqrt(U * np.var(d, ddof=1))) if U > 1 else 0.0, unit=wa.unit, nUnits=U)


def compareLoo(A, B) -> dict:
    """compareWaic on two OutputLoo results (getLooMarginal(..., pointwise=True)), or on two samplers, for which getLooMarginal is called."""
    la = A if isinstance(A, OutputLoo) else getLooMarginal(A, pointwise=True)
    lb = B if isinstance(B, OutputLoo) else getLooMarginal(B, pointwise=True)
    return compareWaic(la, lb)


# ------------------------------------------------------------------------------------------------------------------
# Marginal WAIC (include/ertirt.h: erm_get_marginal_waic).  Unit = a subject with theta_i and zeta_i integrated out: zeta analytically, theta by a fixed
# rule of equally spaced nodes over mu +- 6 sd of the population law.  l_i^(s) depends on row s of the item-level trace only, so it is computed after the run.
# ------------------------------------------------------------------------------------------------------------------
MARGINAL_UNIT = "subject-marginal"


def _marginal_source(MCMC, who="getWaicMarginal"):
    src = getattr(MCMC, "farm", None) or MCMC._engine
    if src is None:
        raise ValueError(f"run sample! first ({who} reads the engine's resident item trace and data set)")
    return src


def _marginal_check(MCMC, nodes, who="getWaicMarginal"):
    if MCMC._model not in _lib.MARGINAL_MODELS:
        raise ValueError(f"{who} is not available for {type(MCMC).__name__}: with the quantile weights integrated out the response-time term is not Gaussian in "
                         "zeta (GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)")
    if MCMC.shard is not None:
        raise ValueError(f"{who} is not available for a subject-sharded sampler (every subject's data must be resident on one device)")
    return _lib.marginal_nodes(nodes)


def getWaicMarginal(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputWaic:
    """Marginal WAIC of the last sample! -- of one engine or of the chain farm of sample!(...; devices=), whose chains' post-burn-in rows enter as one table --
    computed on the device from the resident item trace and data set (erm_get_marginal_waic / erm_farm_get_marginal_waic); needs no waic= at sample!.
    unit = "subject-marginal"; nNodes = nodes, nCoarse = the subjects for which the rule was too coarse at some row (raise nodes if it is not 0).
    pointwise=True also fetches lppd_i and p_i, which compareWaic needs."""
    Q = _marginal_check(MCMC, nodes)
    r = _marginal_source(MCMC).marginal_waic(Q, pointwise=pointwise)
    w, lppd_u, p_u = r if pointwise else (r, None, None)
    return OutputWaic(elpd=w["elpd"], pWaic=w["pWaic"], WAIC=w["WAIC"], se=w["se"], nHighVar=w["nHighVar"], lppd=w["lppd"], unit=MARGINAL_UNIT, nUnits=w["nUnits"],
                      nRows=w["nRows"], lppd_u=lppd_u, p_u=p_u, nNodes=w["nNodes"], nCoarse=w["nCoarse"])


def _marginal_rows_host(model, Y, logT, X, rows, Q):
    """The rule at every row for marginalLogLikHost and scoresHost: yields (e (N, Q), z (Q,), law, sums) with law = (mu (N,), sd, m0, m1, v) and
    sums = (P, R0 (N,), R1) of include/ertirt.h's definition (None for GibbsMlIrt)."""
    t = _lib.MODEL_TRAITS[model]
    Y = np.asarray(Y, dtype=np.float64)
    N, J = Y.shape
    F = 0 if X is None or not t.sees_x else np.shape(X)[1]
    x1 = np.ones((N, 1)) if F == 0 else np.hstack([np.ones((N, 1)), np.asarray(X, dtype=np.float64)])
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if rows.shape[1] != _lib.item_trace_width(model, J, F):
        raise ValueError(f"rows must have {_lib.item_trace_width(model, J, F)} columns")
    h = 12.0 / (Q - 1)
    z = -6.0 + h * np.arange(Q)
    zero = np.zeros(N)
    for row in rows:
        a, b, lam, sg, q = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J], row[4 * J:]
        rho = q[:J] if t.rho else np.zeros(J)
        m0, m1, v = zero, 0.0, 0.0
        if model == _lib.MODEL_MLIRT:
            mu, s11 = x1 @ q[:F + 1], 1.0
        else:
            Sp = q[len(q) - 4:]
            s11, s12, s22 = Sp[0], 0.5 * (Sp[1] + Sp[2]), Sp[3]
            if model == _lib.MODEL_RTIRT:
                mu = x1 @ q[:F + 1]
                m1 = s12 / s11
                m0, v = x1 @ q[F + 1:2 * F + 2] - m1 * mu, s22 - s12 * s12 / s11
            elif model == _lib.MODEL_LATENT:
                mu, m0, m1, v = zero, x1 @ q[:F + 1], q[F + 1], s22
            else:
                mu, m0, m1, v = zero, zero, s12 / s11, s22 - s12 * s12 / s11
        th = mu[:, None] + np.sqrt(s11) * z[None, :]                                  # (N, Q)
        eta = a[None, None, :] * (th[:, :, None] - b[None, None, :])                  # (N, Q, J)
        e = np.log(h) - 0.5 * np.log(2 * np.pi) - 0.5 * z[None, :] ** 2 + np.sum(Y[:, None, :] * eta - _log1pexp(eta), axis=2)
        sums = None
        if t.rt:
            g = 1.0 / sg
            lt = np.asarray(logT, dtype=np.float64)
            d = lam[None, None, :] - lt[:, None, :] - rho[None, None, :] * th[:, :, None]
            P, R, D = np.sum(g), np.sum(g * d, axis=2), np.sum(g * d * d, axis=2)
            m = np.asarray(m0)[:, None] + m1 * th if np.ndim(m0) else m0 + m1 * th
            e = e - 0.5 * J * np.log(2 * np.pi) - 0.5 * np.sum(np.log(sg)) - 0.5 * np.log1p(v * P) - 0.5 * (D + (P * m * m - 2 * R * m - v * R * R) / (1 + v * P))
            sums = (P, np.sum(g[None, :] * (lam[None, :] - lt), axis=1), np.sum(g * rho))
        yield e, z, (mu, np.sqrt(s11), m0, m1, v), sums


def marginalLogLikHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, with_S=False) -> np.ndarray:
    """l_i^(s) of the marginal WAIC with numpy (the test twin of marginal_kernel): an (R, N) array for the item-trace rows [R, item_trace_width] (as
    Engine.item_trace() returns them) and the data Y, logT [N, J], X [N, F] or None.  with_S=True also returns S = sum_q exp(e_q - max_q e_q) per (row, subject):
    S < 2 marks a posterior too narrow for the rule."""
    from scipy.special import logsumexp
    Q = _lib.marginal_nodes(nodes)
    per = [(logsumexp(e, axis=1), np.sum(np.exp(e - np.max(e, axis=1, keepdims=True)), axis=1)) for e, _, _, _ in _marginal_rows_host(model, Y, logT, X, rows, Q)]
    out, outS = np.array([p[0] for p in per]), np.array([p[1] for p in per])
    return (out, outS) if with_S else out


def waicFromLogLik(L, unit=MARGINAL_UNIT, **extra) -> OutputWaic:
    """WAIC from an (|S|, U) array of pointwise log-likelihoods with scipy's logsumexp and np.var(ddof=1), as getWaicHost forms it."""
    from scipy.special import logsumexp
    L = np.asarray(L, dtype=np.float64)
    S, U = L.shape
    if S < 2:
        raise ValueError("WAIC needs at least two post-burn-in rows")
    lppd_u = logsumexp(L, axis=0) - np.log(S)
    p_u = np.var(L, axis=0, ddof=1)
    el = lppd_u - p_u
    elpd = float(np.sum(el))
    se = 2.0 * float(np.sqrt(U * np.var(el, ddof=1))) if U > 1 else 0.0
    return OutputWaic(elpd=elpd, pWaic=float(np.sum(p_u)), WAIC=-2.0 * elpd, se=se, nHighVar=int(np.sum(p_u > 0.4)), lppd=float(np.sum(lppd_u)), unit=unit, nUnits=U,
                      nRows=S, lppd_u=lppd_u, p_u=p_u, **extra)


def marginalRows(MCMC: _GibbsBase) -> np.ndarray:
    """The rows behind getWaicMarginal: the post-burn-in rows of the item-level trace (one engine: rows >= nBurnin * nChain; a chain farm: those of chain 0, then
    chain 1, ...)."""
    src, C = _marginal_source(MCMC), MCMC.Cond
    if getattr(MCMC, "farm", None) is not None:
        return np.concatenate([src.engine(l).item_trace()[C.nBurnin:] for l in range(src.n_chains)], axis=0)
    return src.item_trace()[C.nBurnin * C.nChain:]


def _marginal_loglik_host(MCMC, nodes, rows, who):
    """What getWaicMarginalHost and getLooMarginalHost start from: marginalLogLikHost's l [S, N], the node count, the subjects with a grid too coarse at any row."""
    Q = _marginal_check(MCMC, nodes, who)
    D, t = MCMC.Data, MCMC._traits
    if D is None:
        raise ValueError("Data is required")
    rows = marginalRows(MCMC) if rows is None else rows
    X = np.asarray(D.X, dtype=np.float64) if t.sees_x and MCMC.Cond.nFeat > 0 else None
    L, S = marginalLogLikHost(MCMC._model, D.Y, D.logT if t.rt else None, X, rows, Q, with_S=True)
    return L, Q, int(np.sum(np.any(S < 2.0, axis=0)))


def getWaicMarginalHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputWaic:
    """getWaicMarginal evaluated with numpy / scipy on the host (the test twin of the device path) from MCMC.Data and the item-level trace rows (marginalRows, or
    `rows`)."""
    L, Q, n_coarse = _marginal_loglik_host(MCMC, nodes, rows, "getWaicMarginal")
    return waicFromLogLik(L, nNodes=Q, nCoarse=n_coarse)


# ------------------------------------------------------------------------------------------------------------------
# Marginal WAIC and PSIS-LOO of GibbsRtIrtLatentQr (include/ertirt.h: erm_get_quantile_marginal_waic).  Unit = a subject with theta_i, zeta_i and the
# quantile weight nu_i integrated out: nu turns zeta's law into an asymmetric Laplace one, zeta then integrates to two normal-CDF terms, theta goes by the same rule.
# ------------------------------------------------------------------------------------------------------------------
_QMARG_SERIES_X = -36.0


def _qmarg_log_ndtr(x):
    """log Phi(x) in the three arms of csrc/erm_qmarginal.hpp (qmarg_log_ndtr), restated with scipy's erfc: x >= 0: log1p(-erfc(x / sqrt 2) / 2);
    -36 <= x < 0: log(erfc(-x / sqrt 2) / 2); x < -36: -x^2 / 2 - log(-x) - 1/2 log 2 pi + log1p(-r + 3 r^2 - ... + 2027025 r^8), r = 1 / x^2."""
    from scipy.special import erfc
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    hi, lo = x >= 0.0, x < _QMARG_SERIES_X
    mid = ~hi & ~lo
    out[hi] = np.log1p(-0.5 * erfc(x[hi] * np.sqrt(0.5)))
    out[mid] = np.log(0.5 * erfc(-x[mid] * np.sqrt(0.5)))
    xl = x[lo]
    r = 1.0 / (xl * xl)
    p = np.full_like(r, 2027025.0)
    for c in (-135135.0, 10395.0, -945.0, 105.0, -15.0, 3.0, -1.0):
        p = c + r * p
    out[lo] = -0.5 * xl * xl - np.log(-xl) - 0.5 * np.log(2 * np.pi) + np.log1p(r * p)
    return out


def _qmarginal_check(MCMC, nodes, who):
    if MCMC._model not in _lib.QUANTILE_MARGINAL_MODELS:
        if MCMC._model in _lib.MARGINAL_MODELS:
            raise ValueError(f"{who} is for GibbsRtIrtLatentQr: {type(MCMC).__name__} has no quantile weights, use {who[:-2]}")
        raise ValueError(f"{who} is not available for {type(MCMC).__name__}: with the quantile weights nu_ij integrated out every cell's response time is asymmetric "
                         "Laplace in zeta, and the zeta integral (J kinks that move with theta) has no closed form")
    if MCMC.shard is not None:
        raise ValueError(f"{who} is not available for a subject-sharded sampler (every subject's data must be resident on one device)")
    return _lib.marginal_nodes(nodes)


def quantileMarginalLogLikHost(model, Y, logT, X, rows, qRt, nodes=_lib.MARGINAL_NODES, with_S=False) -> np.ndarray:
    """l_i^(s) of GibbsRtIrtLatentQr's marginal WAIC with numpy (the test twin of marginal_kernel<LATENTQR>): an (R, N) array for the item-trace rows
    [R, item_trace_width] (Latent's layout) and the data Y, logT [N, J], X [N, F] or None at the quantile level qRt.  include/ertirt.h's definition restated:
    theta by the rule of marginalLogLikHost, zeta | theta asymmetric Laplace (m0 + m1 theta, s = Sigma_p[2,2], qRt) integrated against the Gaussian response times
    in closed form.  with_S=True also returns S per (row, subject)."""
    from scipy.special import logsumexp
    if model not in _lib.QUANTILE_MARGINAL_MODELS:
        raise ValueError("quantileMarginalLogLikHost serves GibbsRtIrtLatentQr only")
    q = float(qRt)
    if not 0.0 < q < 1.0:
        raise ValueError("qRt must be inside (0, 1)")
    Q = _lib.marginal_nodes(nodes)
    Y = np.asarray(Y, dtype=np.float64)
    lt = np.asarray(logT, dtype=np.float64)
    N, J = Y.shape
    F = 0 if X is None else np.shape(X)[1]
    x1 = np.ones((N, 1)) if F == 0 else np.hstack([np.ones((N, 1)), np.asarray(X, dtype=np.float64)])
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if rows.shape[1] != _lib.item_trace_width(model, J, F):
        raise ValueError(f"rows must have {_lib.item_trace_width(model, J, F)} columns")
    h = 12.0 / (Q - 1)
    z = -6.0 + h * np.arange(Q)
    out, outS = np.empty((rows.shape[0], N)), np.empty((rows.shape[0], N))
    for r, row in enumerate(rows):
        a, b, lam, sg, qq = row[:J], row[J:2 * J], row[2 * J:3 * J], row[3 * J:4 * J], row[4 * J:]
        s11, s = qq[-4], qq[-1]
        if not (s > 0.0 and s11 > 0.0 and np.all(sg > 0.0)):
            raise ValueError(f"row {r}: sig2t, Sigma_p[1,1] and Sigma_p[2,2] must be positive")
        m0, m1 = x1 @ qq[:F + 1], qq[F + 1]
        th = np.sqrt(s11) * z                                                         # (Q,)
        eta = a[None, None, :] * (th[None, :, None] - b[None, None, :])               # (1, Q, J)
        e = np.log(h) - 0.5 * np.log(2 * np.pi) - 0.5 * z[None, :] ** 2 + np.sum(Y[:, None, :] * eta - _log1pexp(eta), axis=2)
        g = 1.0 / sg
        d0 = lam[None, :] - lt
        P, R0, D0, L = np.sum(g), np.sum(g * d0, axis=1)[:, None], np.sum(g * d0 * d0, axis=1)[:, None], np.sum(np.log(sg))
        m = m0[:, None] + m1 * th[None, :]                                            # (N, Q)
        bU, bL, rP = R0 - q / s, R0 + (1.0 - q) / s, np.sqrt(P)
        up = bU * bU / (2.0 * P) + q * m / s + _qmarg_log_ndtr(-(m - bU / P) * rP)
        lo = bL * bL / (2.0 * P) - (1.0 - q) * m / s + _qmarg_log_ndtr((m - bL / P) * rP)
        e = e - 0.5 * J * np.log(2 * np.pi) - 0.5 * L - 0.5 * D0 + np.log(q * (1.0 - q) / s) + 0.5 * (np.log(2 * np.pi) - np.log(P)) + np.logaddexp(up, lo)
        out[r], outS[r] = logsumexp(e, axis=1), np.sum(np.exp(e - np.max(e, axis=1, keepdims=True)), axis=1)
    return (out, outS) if with_S else out


def getWaicMarginalQr(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputWaic:
    """getWaicMarginal for GibbsRtIrtLatentQr (= GibbsRtIrtQuantile): the marginal WAIC with every subject's theta, zeta and quantile weight nu integrated out, at the
    sampler's qRt, computed on the device (erm_get_quantile_marginal_waic / erm_farm_get_quantile_marginal_waic).  unit = "subject-marginal", so compareWaic takes
    it against a GibbsRtIrtLatent fit of the same data, or against another qRt."""
    Q = _qmarginal_check(MCMC, nodes, "getWaicMarginalQr")
    r = _marginal_source(MCMC, "getWaicMarginalQr").quantile_marginal_waic(Q, pointwise=pointwise)
    w, lppd_u, p_u = r if pointwise else (r, None, None)
    return OutputWaic(elpd=w["elpd"], pWaic=w["pWaic"], WAIC=w["WAIC"], se=w["se"], nHighVar=w["nHighVar"], lppd=w["lppd"], unit=MARGINAL_UNIT, nUnits=w["nUnits"],
                      nRows=w["nRows"], lppd_u=lppd_u, p_u=p_u, nNodes=w["nNodes"], nCoarse=w["nCoarse"])


def getLooMarginalQr(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputLoo:
    """getLooMarginal for GibbsRtIrtLatentQr: PSIS-LOO on the marginal log-likelihoods of getWaicMarginalQr, computed on the device
    (erm_get_quantile_marginal_loo / erm_farm_get_quantile_marginal_loo).  Needs 25 .. 8192 post-burn-in rows."""
    Q = _qmarginal_check(MCMC, nodes, "getLooMarginalQr")
    _lib.psis_rows(_loo_rows(MCMC))
    return _loo_output(_marginal_source(MCMC, "getLooMarginalQr").quantile_marginal_loo(Q, pointwise=pointwise), pointwise)


def _qmarginal_loglik_host(MCMC, nodes, rows, who):
    Q = _qmarginal_check(MCMC, nodes, who)
    D = MCMC.Data
    if D is None:
        raise ValueError("Data is required")
    rows = marginalRows(MCMC) if rows is None else rows
    X = np.asarray(D.X, dtype=np.float64) if MCMC.Cond.nFeat > 0 else None
    L, S = quantileMarginalLogLikHost(MCMC._model, D.Y, D.logT, X, rows, MCMC.Cond.qRt, Q, with_S=True)
    return L, Q, int(np.sum(np.any(S < 2.0, axis=0)))


def getWaicMarginalQrHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputWaic:
    """getWaicMarginalQr evaluated with numpy / scipy on the host (the test twin of the device path)."""
    L, Q, n_coarse = _qmarginal_loglik_host(MCMC, nodes, rows, "getWaicMarginalQr")
    return waicFromLogLik(L, nNodes=Q, nCoarse=n_coarse)


def getLooMarginalQrHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputLoo:
    """getLooMarginalQr evaluated with numpy on the host: quantileMarginalLogLikHost, then psisLooHost."""
    L, Q, n_coarse = _qmarginal_loglik_host(MCMC, nodes, rows, "getLooMarginalQr")
    out = psisLooHost(L)
    out.unit, out.nNodes, out.nCoarse = MARGINAL_UNIT, Q, n_coarse
    return out


# ------------------------------------------------------------------------------------------------------------------
# Marginal PSIS-LOO (include/ertirt.h: erm_get_marginal_loo).  Pareto-smoothed importance-sampling leave-one-subject-out on the marginal
# log-likelihoods l_i^(s) of the marginal WAIC, with the Pareto k^ of every respondent.
# ------------------------------------------------------------------------------------------------------------------
def _loo_output(r, pointwise) -> OutputLoo:
    g = (lambda k: r[k]) if pointwise else (lambda k: None)
    return OutputLoo(elpd=r["elpd"], pLoo=r["pLoo"], LOOIC=r["LOOIC"], se=r["se"], lppd=r["lppd"], unit=MARGINAL_UNIT, nUnits=r["nUnits"], nRows=r["nRows"],
                     nBadK=r["nBadK"], nHighK=r["nHighK"], tailLen=r["tailLen"], elpd_u=g("elpd_u"), p_u=g("p_u"), khat=g("khat"), nEff=g("nEff"),
                     nNodes=r["nNodes"], nCoarse=r["nCoarse"])


def _loo_rows(MCMC):
    """The rows per unit a sampler's getLooMarginal would see, from its conditions alone (no device is touched)."""
    C = MCMC.Cond
    return (C.nIter - C.nBurnin) * C.nChain          # interleaved chains of one engine or the chains of a farm: the same count


def getLooMarginal(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputLoo:
    """Marginal PSIS-LOO of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- computed on the device from the resident item trace
    and data set (erm_get_marginal_loo / erm_farm_get_marginal_loo): Pareto-smoothed leave-one-subject-out with theta_i and zeta_i integrated out, the criterion
    getWaicMarginal's nHighVar points to.  Needs 25 .. 8192 post-burn-in rows.  pointwise=True also fetches elpd_u, p_u, khat and nEff per subject: khat above
    0.7 flags the respondents whose removal would move the posterior (aberrant or highly influential patterns)."""
    Q = _marginal_check(MCMC, nodes, "getLooMarginal")
    _lib.psis_rows(_loo_rows(MCMC))
    return _loo_output(_marginal_source(MCMC, "getLooMarginal").marginal_loo(Q, pointwise=pointwise), pointwise)


def psisLoo(L, device=0, want_lw=False):
    """PSIS-LOO on the device (erm_psis_loo) of a saved table L (|S|, U) of pointwise log-likelihoods, rows in trace order -- marginalLogLikHost's layout; a
    conditional table serves as well.  Returns an OutputLoo with the pointwise vectors (and the smoothed, normalised log-weights (|S|, U) if want_lw)."""
    L = np.asarray(L, dtype=np.float64)
    if L.ndim != 2:
        raise ValueError("L must be (rows, units)")
    _lib.psis_rows(L.shape[0])
    r = _lib.psis_loo(L.T, want_lw=want_lw, device=device)
    out = _loo_output(r, True)
    out.unit = None
    return (out, r["lw"].T) if want_lw else out


def psisTailLen(S) -> int:
    """M = min(ceil(S / 5), ceil(3 sqrt(S))), as the float formula gives it."""
    return int(min(np.ceil(S / 5.0), np.ceil(3.0 * np.sqrt(S))))


def psisLooHost(L, dtype=np.float64, with_lw=False, with_fit=False):
    """PSIS-LOO of an (|S|, U) table of pointwise log-likelihoods with numpy (the test twin of psis_kernel), written from the papers: Vehtari, Gelman and Gabry
    (2017) for the estimator, Vehtari, Simpson, Gelman, Yao and Gabry (2024, Algorithm 1 and Appendix) for the tail length, the smoothing and the k^ prior, Zhang
    and Stephens (2009) for the generalised-Pareto fit; r_eff = 1.  dtype=np.longdouble runs the same arithmetic in extended precision (the tests' measure of the
    computation's own conditioning).  Returns an OutputLoo with the pointwise vectors; with_lw: also the smoothed, normalised log-weights (|S|, U); with_fit: also
    sigma (U,) (NaN where the tail could not be fitted)."""
    from math import floor
    L = np.asarray(L, dtype=dtype)
    if L.ndim != 2:
        raise ValueError("L must be (rows, units)")
    S, U = L.shape
    _lib.psis_rows(S)
    fl = dtype
    M = psisTailLen(S)
    G = 30 + int(floor(np.sqrt(M)))

    def lse(v):
        m = np.max(v)
        return m + np.log(np.sum(np.exp(v - m)))

    elpd, p, khat, neff, sig = (np.empty(U, dtype=fl) for _ in range(5))
    LW = np.empty((S, U), dtype=fl)
    for u in range(U):
        l = L[:, u]
        lw = -l - np.max(-l)
        order = np.argsort(lw, kind="stable")                 # ascending by (lw, position)
        srt = lw[order]
        c = srt[S - M - 1]
        x = np.exp(srt[S - M:]) - np.exp(c)
        k, sigma = fl(np.inf), fl(np.nan)
        xstar = x[int(floor(M / 4 + 0.5)) - 1]
        if xstar > 0 and x[-1] - x[0] > 0:
            with np.errstate(all="ignore"):
                j = np.arange(1, G + 1).astype(fl)
                b = 1 / x[-1] + (1 - np.sqrt(G / (j - fl(0.5)))) / (3 * xstar)
                kj = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
                Lj = M * (np.log(-b / kj) - kj - 1)
                w = np.exp(Lj - lse(Lj))
                bh = np.sum(b * w)
                kr = np.mean(np.log1p(-bh * x))
                sg = -kr / bh
                kh = (M * kr + 5) / fl(M + 10)
            if np.isfinite(bh) and np.isfinite(sg) and np.isfinite(kh):
                k, sigma = kh, sg
        new = srt.copy()
        if np.isfinite(k):
            with np.errstate(all="ignore"):
                pr = (np.arange(1, M + 1).astype(fl) - fl(0.5)) / M
                q = -sigma * np.log1p(-pr) if k == 0 else sigma * np.expm1(-k * np.log1p(-pr)) / k
                new[S - M:] = np.minimum(fl(0), np.log(np.exp(c) + q))
        lwp = np.empty(S, dtype=fl)
        lwp[order] = new
        norm = lse(lwp)
        elpd[u] = lse(lwp + l) - norm
        p[u] = (lse(l) - np.log(fl(S))) - elpd[u]
        khat[u], sig[u] = k, sigma
        wn = np.exp(lwp - norm)
        neff[u] = 1 / np.sum(wn * wn)
        LW[:, u] = lwp - norm
    thr = min(1.0 - 1.0 / np.log10(S), 0.7)
    el = elpd.astype(np.float64)
    se = 2.0 * float(np.sqrt(U * np.var(el, ddof=1))) if U > 1 else 0.0
    out = OutputLoo(elpd=float(np.sum(elpd)), pLoo=float(np.sum(p)), LOOIC=-2.0 * float(np.sum(elpd)), se=se, lppd=float(np.sum(elpd + p)), unit=None, nUnits=U, nRows=S,
                    nBadK=int(np.sum(khat > 0.7)), nHighK=int(np.sum(khat > thr)), tailLen=M, elpd_u=elpd, p_u=p, khat=khat, nEff=neff, nNodes=0, nCoarse=0)
    extra = ([LW] if with_lw else []) + ([sig] if with_fit else [])
    return (out, *extra) if extra else out


def getLooMarginalHost(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, rows=None) -> OutputLoo:
    """getLooMarginal evaluated with numpy on the host (the test twin of the device path): marginalLogLikHost on MCMC.Data and the item-level trace rows
    (marginalRows, or `rows`), then psisLooHost."""
    L, Q, n_coarse = _marginal_loglik_host(MCMC, nodes, rows, "getLooMarginal")
    out = psisLooHost(L)
    out.unit, out.nNodes, out.nCoarse = MARGINAL_UNIT, Q, n_coarse
    return out


# ------------------------------------------------------------------------------------------------------------------
# Scores of respondents (include/ertirt.h: erm_get_scores).  Posterior mean and sd of every subject's theta and zeta from the item-level trace: the
# posterior of theta on the marginal WAIC's rule at every row, zeta given theta Gaussian in closed form, the rows joined by the law of total variance.
# ------------------------------------------------------------------------------------------------------------------
def _scores_output(r, weighting="equal") -> OutputScores:
    return OutputScores(theta=r["theta"], thetaSd=r["thetaSd"], zeta=r["zeta"], zetaSd=r["zetaSd"], cov=r["cov"], rowEss=r["rowEss"], coarse=r["coarse"],
                        nRows=r["nRows"], nNodes=r["nNodes"], nCoarse=r["nCoarse"], weighting=weighting)


def getScores(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES) -> OutputScores:
    """Scores of the subjects of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- computed on the device from the resident item
    trace and data set (erm_get_scores / erm_farm_get_scores), in either trace mode: theta, thetaSd, zeta, zetaSd, cov, rowEss, coarse per subject; relTheta,
    relZeta.  The scores are posterior under the population law of getWaicMarginal: for the response-time models theta borrows strength from the response times, so
    they differ from Post.mean by design (the sampler's theta and zeta draws each use the marginal prior); for GibbsMlIrt the two agree."""
    Q = _marginal_check(MCMC, nodes, "getScores")
    return _scores_output(_marginal_source(MCMC, "getScores").scores(Q))


def scoreRespondents(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal", device=0) -> OutputScores:
    """Scores of respondents -- new ones, or those of a run that is no longer resident -- against saved item-trace rows [R, item_trace_width] (Engine.item_trace()),
    on the device (erm_score).  model: the model code (_lib.MODEL_*); Y, logT [N, J], X [N, F] or None.  weighting "equal": every row counts once, the usual
    operational scoring; "likelihood": row s counts exp(l_s), the posterior of a new respondent given their own data and the saved item posterior."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("scoreRespondents serves the five models without quantile weights")
    w = _lib.score_weighting(weighting)
    return _scores_output(_lib.score(model, Y, logT, X, rows, nodes=_lib.marginal_nodes(nodes), weighting=w, device=device), "likelihood" if w else "equal")


def _row_moments(e, z, law, sums, rt):
    """A row of _marginal_rows_host for scoresHost and plausibleValuesHost: theta's mean and variance E, V (N,) on the rule, zeta | theta ~ N(c0 + c1 theta, u)
    (zeros without response times), the largest e_q, M (N, 1), and the sum s (N,) of exp(e_q - M)."""
    mu, sd, m0, m1, v = law
    M = np.max(e, axis=1, keepdims=True)
    p = np.exp(e - M)
    s = np.sum(p, axis=1)
    w = p / s[:, None]
    Z1, Z2 = w @ z, w @ (z * z)
    E, V = mu + sd * Z1, np.maximum(sd * sd * (Z2 - Z1 * Z1), 0.0)
    c0, c1, u = 0.0, 0.0, 0.0
    if rt:
        P, R0, R1 = sums
        c0, c1, u = (m0 + v * R0) / (1 + v * P), (m1 - v * R1) / (1 + v * P), v / (1 + v * P)
    return E, V, c0, c1, u, M, s


def scoresHost(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal") -> OutputScores:
    """scoreRespondents with numpy (the test twin of score_kernel), written beside marginalLogLikHost: the rule's weights at every row, the moments of theta, the
    zeta conditional, and the rows joined in two passes (the means, then the deviations from them)."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("scoresHost serves the five models without quantile weights")
    Q, wt = _lib.marginal_nodes(nodes), _lib.score_weighting(weighting)
    rt = _lib.MODEL_TRAITS[model].rt
    E, V, Ez, Vz, Cz, l, S = ([] for _ in range(7))
    for e, z, law, sums in _marginal_rows_host(model, Y, logT, X, rows, Q):
        Es, Vs, c0, c1, u, M, s = _row_moments(e, z, law, sums, rt)
        for lst, val in zip((E, V, Ez, Vz, Cz, l, S), (Es, Vs, c0 + c1 * Es, u + c1 * c1 * Vs, c1 * Vs, M[:, 0] + np.log(s), s)):
            lst.append(val)
    E, V, Ez, Vz, Cz, l, S = (np.array(a) for a in (E, V, Ez, Vz, Cz, l, S))             # (R, N)
    om = np.exp(l - np.max(l, axis=0, keepdims=True)) if wt == _lib.SCORE_LIKELIHOOD else np.ones_like(l)
    W = np.sum(om, axis=0)
    mean = lambda a: np.sum(om * a, axis=0) / W
    th, ze = mean(E), mean(Ez)
    nan = np.full(E.shape[1], np.nan)
    coarse = np.any(S < 2.0, axis=0)
    return OutputScores(theta=th, thetaSd=np.sqrt(np.maximum(mean(V) + mean((E - th) ** 2), 0.0)), zeta=ze if rt else nan,
                        zetaSd=np.sqrt(np.maximum(mean(Vz) + mean((Ez - ze) ** 2), 0.0)) if rt else nan, cov=mean(Cz) + mean((E - th) * (Ez - ze)) if rt else nan,
                        rowEss=W * W / np.sum(om * om, axis=0), coarse=coarse, nRows=E.shape[0], nNodes=Q, nCoarse=int(np.sum(coarse)),
                        weighting="likelihood" if wt else "equal")


# ------------------------------------------------------------------------------------------------------------------
# Plausible values (include/ertirt.h: erm_get_plausible_values).  K draws of every subject's (theta, zeta) from its posterior given the item-level
# trace: draw k reads row r_k, picks a node of the marginal WAIC's rule by Gumbel-max on Philox stream 16, spreads theta over the node's cell and shrinks it back to
# the row's mean and variance, and draws zeta from its Gaussian conditional.
# ------------------------------------------------------------------------------------------------------------------
def _pv_output(r) -> OutputPv:
    return OutputPv(theta=r["theta"], zeta=r["zeta"], node=r["node"], coarse=r["coarse"], nRows=r["nRows"], nNodes=r["nNodes"], nCoarse=r["nCoarse"], seed=r["seed"])


def getPlausibleValues(MCMC: _GibbsBase, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES) -> OutputPv:
    """K plausible values per subject of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- drawn on the device from the resident
    item trace and data set (erm_get_plausible_values / erm_farm_get_plausible_values), in either trace mode: theta, zeta (N, K), node, coarse.  Draws from the
    posterior getScores summarises: at every row a draw has the mean and the variance getScores reports there.  The same (K, seed, nodes) gives the same draws."""
    Q = _marginal_check(MCMC, nodes, "getPlausibleValues")
    K, seed = _lib.pv_draws(K), _lib.pv_seed(seed)
    return _pv_output(_marginal_source(MCMC, "getPlausibleValues").plausible_values(K, seed, Q))


def drawPlausibleValues(model, Y, logT, X, rows, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES, device=0) -> OutputPv:
    """Plausible values of respondents -- new ones, or those of a run that is no longer resident -- against saved item-trace rows [R, item_trace_width]
    (Engine.item_trace()), on the device (erm_plausible_values).  model: the model code (_lib.MODEL_*); Y, logT [N, J], X [N, F] or None; every row counts once."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("drawPlausibleValues serves the five models without quantile weights")
    Q, K, seed = _lib.marginal_nodes(nodes), _lib.pv_draws(K), _lib.pv_seed(seed)
    return _pv_output(_lib.plausible_values(model, Y, logT, X, rows, K=K, seed=seed, nodes=Q, device=device))


def pvRow(k, K, n_rows):
    """The row of draw k: ((2 k + 1) n_rows) // (2 K) (pv_row of csrc/erm_pv.hpp)."""
    return ((2 * np.asarray(k, dtype=np.int64) + 1) * np.int64(n_rows)) // np.int64(2 * K)


def pvGumbel(w):
    """The Gumbel variate of a 32-bit word: -log(-log((w + 1/2) 2^-32)) (pv_gumbel)."""
    return -np.log(-np.log(_ppc_uniform(np.asarray(w, dtype=np.uint64))))


def pvFinish(E, V, mu, sd, c0, c1, u, q, h, w0, w1, w2):
    """(theta, zeta) of a draw at node q of a row with moments E, V, law (mu, sd) and zeta conditional (c0, c1, u), from the finishing block's words (pv_finish)."""
    cell = sd * h
    star = (mu + sd * (-6.0 + q * h)) + cell * (_ppc_uniform(w0) - 0.5)
    c = np.where(V > 0.0, np.sqrt(V / (V + cell * cell / 12.0)), 0.0)
    theta = E + c * (star - E)
    return theta, (c0 + c1 * theta) + np.sqrt(u) * _ppc_normal(w1, w2)


def plausibleValuesHost(model, Y, logT, X, rows, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES, i_base=0, with_gap=False, with_rows=False):
    """drawPlausibleValues with numpy (the test twin of pv_kernel), written beside scoresHost on _marginal_rows_host and _philox4x32_10.  i_base: the data-set index
    of Y's first subject.  with_gap=True also returns, per draw, the difference of the two largest keys (N, K): a draw whose gap is below the rounding of e_q is
    undecidable between two implementations.  with_rows=True also returns the rows r_k (K,) and the row moments E, V (N, K) each draw was made from."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("plausibleValuesHost serves the five models without quantile weights")
    Q, K, seed = _lib.marginal_nodes(nodes), _lib.pv_draws(K), _lib.pv_seed(seed)
    rt = _lib.MODEL_TRAITS[model].rt
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    rk = pvRow(np.arange(K), K, rows.shape[0])
    used = np.unique(rk)
    N = np.shape(Y)[0]
    h = 12.0 / (Q - 1)
    ii = (np.arange(N, dtype=np.uint64) + np.uint64(i_base))
    site = _ppc_stream_word3(0, _lib.PV_SITE)
    theta, zeta, node, gap = np.empty((N, K)), np.full((N, K), np.nan), np.empty((N, K), dtype=np.int32), np.empty((N, K))
    Ek, Vk = np.empty((N, K)), np.empty((N, K))
    coarse = np.zeros(N, dtype=bool)
    for r, (e, z, law, sums) in zip(used, _marginal_rows_host(model, Y, logT, X, rows[used], Q)):
        (mu, sd), (E, V, c0, c1, u, _, s) = law[:2], _row_moments(e, z, law, sums, rt)
        coarse |= s < 2.0
        ks = np.nonzero(rk == r)[0]
        w0 = _philox4x32_10(ii[:, None, None], ks[None, :, None], np.arange(Q)[None, None, :], site, seed, seed >> 32)[0]      # (N, draws, Q)
        key = e[:, None, :] + pvGumbel(w0)
        q = np.argmax(key, axis=2)                                                                                           # the first of equal keys: the smaller q
        top = np.sort(key, axis=2)
        f0, f1, f2, _ = _philox4x32_10(ii[:, None], ks[None, :], 0xFFFFFFFF, site, seed, seed >> 32)                        # (N, draws)
        col = lambda a: a[:, None] if np.ndim(a) else a
        th, ze = pvFinish(col(E), col(V), col(mu), sd, col(c0), col(c1), u, q, h, f0, f1, f2)
        theta[:, ks], node[:, ks], gap[:, ks] = th, q, top[:, :, -1] - top[:, :, -2]
        Ek[:, ks], Vk[:, ks] = col(E), col(V)
        if rt:
            zeta[:, ks] = ze
    out = OutputPv(theta=theta, zeta=zeta, node=node, coarse=coarse, nRows=rows.shape[0], nNodes=Q, nCoarse=int(np.sum(coarse)), seed=seed)
    extra = ((gap,) if with_gap else ()) + ((rk, Ek, Vk),) * bool(with_rows)
    return (out, *extra) if extra else out


# ------------------------------------------------------------------------------------------------------------------
# Posterior predictive checks.  At every replicate row the data set is drawn again from the model at the values of that row; the deviance of the
# responses, the chi^2 of the response times and the item scores of the replicate are compared with those of the data, per subject, per item and over the data set.
# ------------------------------------------------------------------------------------------------------------------
def getPpc(MCMC: _GibbsBase) -> OutputPpc:
    """Posterior predictive checks of the last sample!(...; ppc=True | thin), from the accumulators the engine kept on the device (erm_get_predictive)."""
    if getattr(MCMC, "farm", None) is not None:
        raise ValueError("getPpc is not available for a sampler run through devices= (a chain farm keeps no predictive accumulators)")
    eng, thin = MCMC._engine, getattr(MCMC, "_ppc_thin", 0)
    if eng is None or not thin:
        raise ValueError("run sample!(...; ppc=True) first (getPpc reads the engine's resident accumulators)")
    item, subj, total = eng.predictive()
    return OutputPpc(R=eng.predictive_reps, thin=thin, item=item, subj=subj, total=total)


_PPC_SITE = 14          # the replicate draws' stream site (erm_predictive_kernels.hpp: SITE_PRED)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on broadcastable arrays of 32-bit counter and key words; returns the four output words as uint64 arrays < 2^32."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _ppc_uniform(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def _ppc_normal(wa, wb):
    return np.sqrt(-2.0 * np.log(_ppc_uniform(wa))) * np.cos(2.0 * np.pi * _ppc_uniform(wb))


def _ppc_stream_word3(chain, site=_PPC_SITE, k=0):
    return (site << 24) | ((chain & 0xFF) << 16) | k


def getPpcHost(MCMC: _GibbsBase, thin=1, sweep0=1, *, seed=None, chain=None, row_base=0) -> OutputPpc:
    """getPpc evaluated with numpy on the host from MCMC.Data and the full Post traces (the test twin of the device path): the same replicate draws -- one
    Philox4x32-10 block per cell at (site 14, subject, item, sweep, chain) -- and the same discrepancies.  sweep0: the global sweep index of trace row 0 (1 on a
    fresh engine or after setSeed; it goes on counting over erm_reset_trace).  The result also carries `margin`: per unit and component the smallest non-zero
    |D_rep - D_obs| over the replicate rows relative to the magnitudes compared (a count is decided beyond rounding when its margin is far above 1e-16)."""
    C, D, P, m = MCMC.Cond, MCMC.Data, MCMC.Post, MCMC._model
    N, J = C.nSubj, C.nItem
    if thin < 1:
        raise ValueError("thin must be at least 1")
    if np.ndim(P.ra) != 3:
        raise ValueError("getPpcHost needs the full Post traces (trace='full' and fill=True)")
    seed = int(MCMC.seed if seed is None else seed)
    chain = int(getattr(MCMC, "chain_id", 0) if chain is None else chain)
    Y = np.asarray(D.Y, dtype=np.float64)
    rt_model = m != _lib.MODEL_MLIRT
    logT = np.asarray(D.logT, dtype=np.float64) if rt_model else None
    q = C.qRt
    k1, k2 = ((1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))) if m == _lib.MODEL_CROSSQR else (0.0, 1.0)
    if m == _lib.MODEL_CROSSQR and P.qr.shape[1] != J + 4 + N * J:
        raise ValueError("getPpcHost needs the per-sweep nu trace of GibbsRtIrtCrossQr in Post.qr")
    ii, jj = np.arange(N, dtype=np.uint64)[:, None] + np.uint64(row_base), np.arange(J, dtype=np.uint64)[None, :]
    item, subj, total = np.zeros((3, 4, J)), np.zeros((2, 4, N)), np.zeros((2, 4))
    margin = dict(item=np.full((3, J), np.inf), subject=np.full((2, N), np.inf), total=np.full(2, np.inf))
    if not rt_model:
        item[1], subj[1], total[1] = np.nan, np.nan, np.nan

    def update(acc, mar, obs, rep, diff, scale):
        acc[0] += diff >= 0
        acc[1] += diff > 0
        acc[2] += obs
        acc[3] += rep
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(diff != 0, np.abs(diff) / scale, np.inf)
        np.minimum(mar, rel, out=mar)

    R = 0
    post = [(it, l) for it in range(C.nBurnin, C.nIter) for l in range(C.nChain)]
    for k, (it, l) in enumerate(post):
        if k % thin:
            continue
        R += 1
        sweep = sweep0 + it * C.nChain + l
        ra = P.ra[it, :, l]
        th, a, b = ra[:N], ra[N:N + J], ra[N + J:N + 2 * J]
        eta = a[None, :] * (th[:, None] - b[None, :])
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-eta))
        w0, w1, w2, _ = _philox4x32_10(ii, jj, sweep, _ppc_stream_word3(chain), seed, seed >> 32)
        yrep = (_ppc_uniform(w0) < p).astype(np.float64)
        lobs = Y * eta - _log1pexp(eta)
        dcell = (Y - yrep) * eta                        # l(y) - l(y_rep): D_rep - D_obs = 2 sum dcell
        for ax, acc, mar in ((1, subj, margin["subject"]), (0, item, margin["item"]), (None, total, margin["total"])):
            dobs, dlt = -2.0 * lobs.sum(axis=ax), dcell.sum(axis=ax)
            update(acc[0], mar[0] if ax is not None else mar[0:1], dobs, dobs + 2.0 * dlt, dlt, np.abs(dcell).sum(axis=ax))
        tobs, trep = Y.sum(axis=0), yrep.sum(axis=0)
        update(item[2], margin["item"][2], tobs, trep, trep - tobs, 1.0)
        if rt_model:
            rt = P.rt[it, :, l]
            ze, lam, sg = rt[:N], rt[N:N + J], rt[N + J:N + 2 * J]
            mu = lam[None, :] - ze[:, None]
            var = np.broadcast_to(sg[None, :], (N, J))
            if m in (_lib.MODEL_CROSS, _lib.MODEL_CROSSQR):
                qr = P.qr[it, :, l]
                mu = mu - th[:, None] * qr[None, :J]
                if m == _lib.MODEL_CROSSQR:
                    nu = qr[J + 4:].reshape(N, J, order="F")
                    mu = mu + k1 * nu
                    var = sg[None, :] * (k2 * nu)
            z = _ppc_normal(w1, w2)                     # logT_rep = mu + sqrt(var) z: its standardised square is z^2
            cobs, crep = (logT - mu) ** 2 / var, z * z
            for ax, acc, mar in ((1, subj, margin["subject"]), (0, item, margin["item"]), (None, total, margin["total"])):
                o, r_ = cobs.sum(axis=ax), crep.sum(axis=ax)
                update(acc[1], mar[1] if ax is not None else mar[1:2], o, r_, r_ - o, o + r_)
    if R == 0:
        raise ValueError("posterior predictive checks need at least one replicate row")
    for acc in (item, subj, total):
        acc[:, 2:4] /= R
    out = OutputPpc(R=R, thin=thin, item=item, subj=subj, total=total)
    out.margin = margin
    return out


def ess_rhat(x: np.ndarray):
    """Split-R-hat and effective sample size (Geyer's initial monotone sequence over the split chains; BDA3 sec. 11.4-11.5, the
    non-rank-normalised estimator) of draws x[(iteration, chain)] -- the host twin of the device kernel `diag_kernel`, used by its
    tests and for traces that are not resident on the device.  A column that never moves -- every used draw (the first and last
    floor(T / 2) of every chain) equal to the first one -- gets (nan, nan); a column whose first pair sum rho_0 + rho_1 is not positive gets
    ess = -M n (M = 2 * chains sequences of n draws): the sum of pair sums stops before it (and pair sums that add up to less than 1 / 2 give a negative ess)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, C = x.shape
    n = T // 2
    seq = np.stack([x[:n, l] if h == 0 else x[T - n:, l] for l in range(C) for h in (0, 1)])      # (M, n)
    M = seq.shape[0]
    if not np.any(seq != seq[0, 0]):          # decided on the draws: the rounded mean of n copies of 0.1 is not 0.1, and W > 0 would be rounding noise
        return float("nan"), float("nan")
    mu = seq.mean(axis=1)
    d = seq - mu[:, None]
    W = np.mean(np.sum(d * d, axis=1) / (n - 1))
    Bn = np.sum((mu - mu.mean()) ** 2) / (M - 1)
    varp = W * (n - 1) / n + Bn

    def rho(t):
        return 1.0 - (W - np.mean(np.sum(d[:, :n - t] * d[:, t:], axis=1) / n)) / varp

    total, prev, t = 0.0, np.inf, 0
    while t + 1 < n:
        P = rho(t) + rho(t + 1)
        if not P > 0:
            break
        P = min(P, prev)
        prev = P
        total += P
        t += 2
    return M * n / (-1.0 + 2.0 * total), float(np.sqrt(varp / W))


def rank_ess_rhat(x: np.ndarray):
    """(ess_bulk, ess_tail, rhat_rank) of draws x[(iteration, chain)]: the rank-normalised diagnostics of Vehtari et al. (2021) as include/ertirt.h defines them
    for erm_get_rank_diagnostics -- the host twin of the device kernel `rank_diag_kernel`, on numpy / scipy.  The used draws are ess_rhat's (the first and last
    floor(T / 2) of every chain), pooled: z = ndtri((average rank - 3/8) / (S + 1/4)), ess_bulk = E(z); f = |x - med| with med the mean of the two middle order
    statistics, rhat_rank = the larger of R(z) and R(z(f)) (R(z) alone when f is constant); with k = ceil(S / 20), ess_tail = the smaller of E([x <= x_(k)]) and
    E([x >= x_(S+1-k)]), NaN if either indicator is constant.  E and R are ess_rhat's.  A column that never moves gets three NaN."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, C = x.shape
    n = T // 2
    u = np.concatenate([x[:n], x[T - n:]], axis=0)                # the used draws [2 n, chain]: ess_rhat splits them exactly as it splits x
    S = u.size
    nan = float("nan")
    if not np.any(u != u[0, 0]):
        return nan, nan, nan

    def scores(v):
        return ndtri((rankdata(v.ravel(), method="average").reshape(v.shape) - 0.375) / (S + 0.25))

    srt = np.sort(u.ravel())
    k = (S + 19) // 20
    ess_bulk, rz = ess_rhat(scores(u))
    med = 0.5 * (srt[S // 2 - 1] + srt[S // 2])
    _, rf = ess_rhat(scores(np.abs(u - med)))
    el, _ = ess_rhat((u <= srt[k - 1]).astype(np.float64))
    eu, _ = ess_rhat((u >= srt[S - k]).astype(np.float64))
    ess_tail = nan if (np.isnan(el) or np.isnan(eu)) else min(el, eu)
    return ess_bulk, ess_tail, (rf if (not np.isnan(rf) and rf > rz) else rz)


def _diag_source(MCMC):
    """What checkConvergence reads: the chain farm of the last sample!(...; devices=) -- its JOINT diagnostics over all chains (erm_farm_get_diagnostics and its
    siblings) -- else the sampler's engine, as getDic chooses."""
    src = getattr(MCMC, "farm", None) or MCMC._engine
    if src is None:
        raise ValueError("run sample! first")
    return src


# checkConvergence's two kinds: the source's (vectors, counts) method pair and the result's keys -- one (share, "ok / n") pair per (defined, converged) pair
# of counters, in the counters' order
_CONVERGENCE_KINDS = {"basic": ("diagnostics", "convergence", (("ess", "essN"), ("rhat", "rhatN"))),
                      "rank": ("rank_diagnostics", "rank_convergence", (("ess", "essN"), ("essTail", "essTailN"), ("rhat", "rhatN")))}


def checkConvergence(MCMC: _GibbsBase, *, detail=True, kind="basic") -> dict:
    """src/SimTools.jl:419-443: share of the ra / rt / qr columns with ESS > 400 and R-hat < 1.1 after burn-in.  The reference runs
    MCMCChains' `ess_rhat` on the host; here both statistics come from the device-resident traces.  kind="basic" (the default): erm_get_diagnostics, split-R-hat and
    Geyer's initial-monotone-sequence ESS, not rank-normalised.  kind="rank": erm_get_rank_diagnostics, the rank-normalised estimator of Vehtari et al. (2021)
    that MCMCChains 6 reports -- `ess` is then the share by bulk-ESS, `essTail` the share by tail-ESS, `rhat` the share by rank-normalised R-hat (with `essN`,
    `essTailN`, `rhatN`), and with detail=True every trace carries (ess_bulk, ess_tail, rhat_rank).  Columns that
    never move (NaN) are left out of the denominators, as the reference does for qr.  detail=False also COUNTS on the device
    (erm_get_convergence / erm_get_rank_convergence): eight (eighteen) integers cross the boundary instead of the N-wide vectors.
    After sample!(...; devices=) the statistics are the chain farm's: every estimator over the nChain independent chains jointly (erm_farm_get_diagnostics and its
    siblings, computed on the first chain's device), which is where R-hat sees the variance between chains."""
    eng = _diag_source(MCMC)
    if kind not in _CONVERGENCE_KINDS:
        raise ValueError('kind must be "basic" or "rank"')
    vectors, counts, keys = _CONVERGENCE_KINDS[kind]
    tot = np.zeros(2 * len(keys), dtype=np.int64)
    out = {}
    for name, which in (("ra", _lib.TRACE_RA), ("rt", _lib.TRACE_RT), ("qr", _lib.TRACE_QR)):
        if which == _lib.TRACE_RT and not MCMC._traits.rt:
            continue
        try:
            if detail:
                out[name] = vec = getattr(eng, vectors)(which)
                with np.errstate(invalid="ignore"):                 # every vector is an ESS (> 400) but the last, the R-hat (< 1.1)
                    c = [n for v in vec[:-1] for n in (np.sum(~np.isnan(v)), np.sum(v > 400))] + [np.sum(~np.isnan(vec[-1])), np.sum(vec[-1] < 1.1)]
            else:
                c = getattr(eng, counts)(which)
        except _lib.ErmError:
            if which != _lib.TRACE_QR:
                raise
            continue                                    # CrossQr without a resident nu trace
        tot += np.asarray(c, dtype=np.int64)
    pairs = [(int(tot[2 * k]), int(tot[2 * k + 1])) for k in range(len(keys))]
    res = {share: 100.0 * ok / max(n, 1) for (share, _), (n, ok) in zip(keys, pairs)}
    res.update({label: f"{ok} / {n}" for (_, label), (n, ok) in zip(keys, pairs)})
    if detail:
        res["detail"] = out
    return res


def coef(MCMC: _GibbsBase) -> dict:
    """Posterior-mean tables of `coef` (src/GibbsRtIrt.pl.jl:479-538) as plain arrays (pretty-printing is out of scope)."""
    C, M = MCMC.Cond, MCMC.Post.mean
    out = {"a": M.a, "b": M.b}
    if MCMC._traits.rt:
        out.update({"λ": M.lam, "σ²t": M.sig2t, "Σp": np.asarray(M.Sigp).reshape(2, 2, order="F")})
    if MCMC._traits.beta in ("pair", "zero_pair"):
        out["β"] = np.asarray(M.beta).reshape(C.nFeat + 1, 2, order="F")
    elif M.beta.size:
        out["β"] = M.beta
    if MCMC._traits.rho:
        out["ρ"] = M.rho
    return out


def precis(MCMC: _GibbsBase) -> dict:
    """Mean / sd / 2.5% / 97.5% of the item-level and structural traces after burn-in (`precis`, src/GibbsRtIrt.pl.jl:545-675,
    without the MCMCChains ESS/R-hat columns)."""
    C = MCMC.Cond
    it = MCMC.Post.item_trace[C.nBurnin * C.nChain:]
    J = C.nItem
    names = [f"a[{j+1}]" for j in range(J)] + [f"b[{j+1}]" for j in range(J)] + [f"λ[{j+1}]" for j in range(J)] + \
            [f"σ²t[{j+1}]" for j in range(J)] + [f"qr[{k+1}]" for k in range(it.shape[1] - 4 * J)]
    return {"names": names, "mean": it.mean(0), "std": it.std(0, ddof=1), "q025": np.quantile(it, 0.025, axis=0),
            "q975": np.quantile(it, 0.975, axis=0)}

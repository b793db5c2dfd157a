"""Sampler objects and `sample!` for the MI355X engine -- host-side mirror of
/root/reference/src/GibbsRtIrt.pl.jl:35-472, src/GibbsRtIrtCross.pl.jl:55-353, src/GibbsRtIrtLatent.pl.jl:50-365.

Same struct names, fields (Cond, Data, truePara, Para, Post), constructor behaviour (always (re)initialises Para and
allocates Post), kwargs and error text as the reference.  `sample!` is spelled `sample_b` (PyJulia's convention for `!`)
and is also exported as `sample`.  All sampling happens in libertirt.so on the GPU; there is no CPU path here.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .base import InputPara, OutputDic, OutputItemFit, OutputLoo, OutputPersonFit, OutputPpc, OutputPv, OutputScores, OutputWaic, SimConditions

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
# For GibbsRtIrtLatentQr (erm_get_quantile_marginal_waic) the quantile weight nu_i is integrated out too: nu turns zeta's law into an asymmetric Laplace
# one, zeta then integrates to two normal-CDF terms, theta goes by the same rule.  The two families are the rows of _lib.MARGINAL_FAMILIES.
# ------------------------------------------------------------------------------------------------------------------
MARGINAL_UNIT = "subject-marginal"


def _marginal_source(MCMC, who="getWaicMarginal"):
    src = getattr(MCMC, "farm", None) or MCMC._engine
    if src is None:
        raise ValueError(f"run sample! first ({who} reads the engine's resident item trace and data set)")
    return src


# Why a family of _lib.MARGINAL_FAMILIES does not serve a sampler whose model is outside its models
_NOT_SERVED = {
    "gaussian": "with the quantile weights integrated out the response-time term is not Gaussian in zeta (GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; "
                "GibbsRtIrtCrossQr: the zeta integral has no closed form)",
    "quantile": "with the quantile weights nu_ij integrated out every cell's response time is asymmetric Laplace in zeta, and the zeta integral (J kinks that move "
                "with theta) has no closed form",
}


def _marginal_check(MCMC, nodes, who="getWaicMarginal", family="gaussian"):
    """Refuse, in `who`'s name, a sampler whose model the family does not serve and a subject-sharded one; returns the node count as the library takes it."""
    if MCMC._model not in _lib.MARGINAL_FAMILIES[family].models:
        if family == "quantile" and MCMC._model in _lib.MARGINAL_MODELS:          # who = the Gaussian getter's name + "Qr"
            raise ValueError(f"{who} is for GibbsRtIrtLatentQr: {type(MCMC).__name__} has no quantile weights, use {who[:-2]}")
        raise ValueError(f"{who} is not available for {type(MCMC).__name__}: {_NOT_SERVED[family]}")
    if MCMC.shard is not None:
        raise ValueError(f"{who} is not available for a subject-sharded sampler (every subject's data must be resident on one device)")
    return _lib.marginal_nodes(nodes)


def _marginal_pass(MCMC, family, product, who, nodes, pointwise):
    """The result of the family's "waic" or "loo" entry of the sampler's engine or farm, after `who`'s checks."""
    Q = _marginal_check(MCMC, nodes, who, family)
    if product == "loo":
        _lib.psis_rows(_loo_rows(MCMC))
    return getattr(_marginal_source(MCMC, who), _lib.MARGINAL_FAMILIES[family].stem + product)(Q, pointwise=pointwise)


def _waic_output(r, pointwise) -> OutputWaic:
    w, lppd_u, p_u = r if pointwise else (r, None, None)
    return OutputWaic(elpd=w["elpd"], pWaic=w["pWaic"], WAIC=w["WAIC"], se=w["se"], nHighVar=w["nHighVar"], lppd=w["lppd"], unit=MARGINAL_UNIT, nUnits=w["nUnits"],
                      nRows=w["nRows"], lppd_u=lppd_u, p_u=p_u, nNodes=w["nNodes"], nCoarse=w["nCoarse"])


def getWaicMarginal(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputWaic:
    """Marginal WAIC of the last sample! -- of one engine or of the chain farm of sample!(...; devices=), whose chains' post-burn-in rows enter as one table --
    computed on the device from the resident item trace and data set (erm_get_marginal_waic / erm_farm_get_marginal_waic); needs no waic= at sample!.
    unit = "subject-marginal"; nNodes = nodes, nCoarse = the subjects for which the rule was too coarse at some row (raise nodes if it is not 0).
    nodes: odd, 3 .. 1025.  The default of 61 suits forms of some tens of items; a form of several hundred items narrows every posterior below the spacing, and
    61 nodes then flag every respondent (at 586, 683 and 896 items of the test data all 40 of 40, S between 1 and 2).  Raise nodes until nCoarse is 0: 255 clears
    it at 896 items on that data (tests/test_item_pass_limits_host.py).
    pointwise=True also fetches lppd_i and p_i, which compareWaic needs."""
    return _waic_output(_marginal_pass(MCMC, "gaussian", "waic", "getWaicMarginal", nodes, pointwise), pointwise)


def getWaicMarginalQr(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputWaic:
    """getWaicMarginal for GibbsRtIrtLatentQr (= GibbsRtIrtQuantile): the marginal WAIC with every subject's theta, zeta and quantile weight nu integrated out, at the
    sampler's qRt, computed on the device (erm_get_quantile_marginal_waic / erm_farm_get_quantile_marginal_waic).  unit = "subject-marginal", so compareWaic takes
    it against a GibbsRtIrtLatent fit of the same data, or against another qRt."""
    return _waic_output(_marginal_pass(MCMC, "quantile", "waic", "getWaicMarginalQr", nodes, pointwise), pointwise)


def marginalRows(MCMC: _GibbsBase) -> np.ndarray:
    """The rows behind getWaicMarginal: the post-burn-in rows of the item-level trace (one engine: rows >= nBurnin * nChain; a chain farm: those of chain 0, then
    chain 1, ...)."""
    src, C = _marginal_source(MCMC), MCMC.Cond
    if getattr(MCMC, "farm", None) is not None:
        return np.concatenate([src.engine(l).item_trace()[C.nBurnin:] for l in range(src.n_chains)], axis=0)
    return src.item_trace()[C.nBurnin * C.nChain:]


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
    return _loo_output(_marginal_pass(MCMC, "gaussian", "loo", "getLooMarginal", nodes, pointwise), pointwise)


def getLooMarginalQr(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES, pointwise=False) -> OutputLoo:
    """getLooMarginal for GibbsRtIrtLatentQr: PSIS-LOO on the marginal log-likelihoods of getWaicMarginalQr, computed on the device
    (erm_get_quantile_marginal_loo / erm_farm_get_quantile_marginal_loo).  Needs 25 .. 8192 post-burn-in rows."""
    return _loo_output(_marginal_pass(MCMC, "quantile", "loo", "getLooMarginalQr", nodes, pointwise), pointwise)


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


# ------------------------------------------------------------------------------------------------------------------
# Scores of respondents (include/ertirt.h: erm_get_scores).  Posterior mean and sd of every subject's theta and zeta from the item-level trace: the
# posterior of theta on the marginal WAIC's rule at every row, zeta given theta Gaussian in closed form, the rows joined by the law of total variance.
# ------------------------------------------------------------------------------------------------------------------
def _scores_output(r, weighting="equal") -> OutputScores:
    return OutputScores(theta=r["theta"], thetaSd=r["thetaSd"], zeta=r["zeta"], zetaSd=r["zetaSd"], cov=r["cov"], rowEss=r["rowEss"], coarse=r["coarse"],
                        nRows=r["nRows"], nNodes=r["nNodes"], nCoarse=r["nCoarse"], weighting=weighting, nObs=r.get("nObs"))


# Incomplete response patterns (include/ertirt.h: erm_score_masked): scoreRespondents and drawPlausibleValues take obs [N, J], 1 = the cell was
# administered.  Calibration keeps its complete-data contract.
def observedMask(Y, logT=None) -> np.ndarray:
    """The observed mask of a data set whose missing cells are marked in the data: uint8 [N, J], 1 where Y is 0 or 1 and logT is finite (logT=None, GibbsMlIrt: Y
    alone).  One bit per cell: a response without a time, or a time without a response, counts as not administered."""
    Y = np.asarray(Y, dtype=np.float64)
    ok = (Y == 0.0) | (Y == 1.0)
    if logT is not None:
        lt = np.asarray(logT, dtype=np.float64)
        if lt.shape != Y.shape:
            raise ValueError("logT does not match Y")
        ok &= np.isfinite(lt)
    return ok.astype(np.uint8)


def _masked_data(Y, logT, obs):
    """Y and logT with the unobserved cells set to 0 (the library never reads them; a NaN in a float Y would not survive the conversion to uint8)."""
    if obs is None:
        return Y, logT
    O = np.asarray(obs) != 0
    if O.shape != np.shape(Y):
        raise ValueError("obs does not match Y")
    return np.where(O, np.asarray(Y), 0), None if logT is None else np.where(O, np.asarray(logT, dtype=np.float64), 0.0)


def getScores(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES) -> OutputScores:
    """Scores of the subjects of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- computed on the device from the resident item
    trace and data set (erm_get_scores / erm_farm_get_scores), in either trace mode: theta, thetaSd, zeta, zetaSd, cov, rowEss, coarse per subject; relTheta,
    relZeta.  The scores are posterior under the population law of getWaicMarginal: for the response-time models theta borrows strength from the response times, so
    they differ from Post.mean by design (the sampler's theta and zeta draws each use the marginal prior); for GibbsMlIrt the two agree.
    nodes: as getWaicMarginal's -- the default of 61 flags every respondent of a form of several hundred items; raise it until nCoarse is 0 (255 at 896 items)."""
    Q = _marginal_check(MCMC, nodes, "getScores")
    return _scores_output(_marginal_source(MCMC, "getScores").scores(Q))


def scoreRespondents(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal", device=0, obs=None) -> OutputScores:
    """Scores of respondents -- new ones, or those of a run that is no longer resident -- against saved item-trace rows [R, item_trace_width] (Engine.item_trace()),
    on the device (erm_score).  model: the model code (_lib.MODEL_*); Y, logT [N, J], X [N, F] or None.  weighting "equal": every row counts once, the usual
    operational scoring; "likelihood": row s counts exp(l_s), the posterior of a new respondent given their own data and the saved item posterior.
    obs [N, J], 0/1 (observedMask builds one): respondents who did not see every item (erm_score_masked) -- every sum over the items runs over the observed cells,
    a respondent with none gets the population law; the result carries nObs, the observed cells per respondent."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("scoreRespondents serves the five models without quantile weights")
    w = _lib.score_weighting(weighting)
    Y, logT = _masked_data(Y, logT, obs)
    return _scores_output(_lib.score(model, Y, logT, X, rows, nodes=_lib.marginal_nodes(nodes), weighting=w, device=device, obs=obs), "likelihood" if w else "equal")


# ------------------------------------------------------------------------------------------------------------------
# Person fit (include/ertirt.h: erm_get_person_fit).  A fit flag beside every score: lz of the responses and the chi^2 of the response times, each
# averaged over the posterior of theta on the marginal WAIC's rule at every row, with posterior predictive p-values.  Deterministic.
# ------------------------------------------------------------------------------------------------------------------
def _fit_output(r, weighting="equal") -> OutputPersonFit:
    return OutputPersonFit(lz=r["lz"], pResp=r["pResp"], ltz=r["ltz"], pTime=r["pTime"], rowEss=r["rowEss"], coarse=r["coarse"], nRows=r["nRows"],
                           nNodes=r["nNodes"], nCoarse=r["nCoarse"], weighting=weighting, nObs=r.get("nObs"))


def getPersonFit(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES) -> OutputPersonFit:
    """Person fit of the subjects of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- computed on the device from the resident
    item trace and data set (erm_get_person_fit / erm_farm_get_person_fit), in either trace mode: lz, pResp, ltz, pTime, rowEss, coarse per subject.  Small pResp:
    the responses are improbable for that person (guessing, pre-knowledge, copying); small pTime: the response times are.  Under the population law of getScores.
    nodes: as getWaicMarginal's."""
    Q = _marginal_check(MCMC, nodes, "getPersonFit")
    return _fit_output(_marginal_source(MCMC, "getPersonFit").person_fit(Q))


def personFit(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, weighting="equal", device=0, obs=None) -> OutputPersonFit:
    """Person fit of respondents -- new ones, or those of a run that is no longer resident -- against saved item-trace rows [R, item_trace_width]
    (Engine.item_trace()), on the device (erm_person_fit); the arguments are scoreRespondents'.  obs [N, J], 0/1: respondents who did not see every item
    (erm_person_fit_masked) -- every sum runs over the observed cells and the chi^2 has n_i degrees of freedom; a respondent with none gets NaN; the result
    carries nObs."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("personFit serves the five models without quantile weights")
    w = _lib.score_weighting(weighting)
    Y, logT = _masked_data(Y, logT, obs)
    return _fit_output(_lib.person_fit(model, Y, logT, X, rows, nodes=_lib.marginal_nodes(nodes), weighting=w, device=device, obs=obs), "likelihood" if w else "equal")


# ------------------------------------------------------------------------------------------------------------------
# Item fit and drift (include/ertirt.h: erm_get_item_fit).  Per item infit, outfit, a signed response residual, a response-time mean square and a
# signed response-time residual: the person fit's cells summed over the subjects instead of the items.  Deterministic; equal row weights.
# ------------------------------------------------------------------------------------------------------------------
def _item_fit_output(r) -> OutputItemFit:
    return OutputItemFit(infit=r["infit"], outfit=r["outfit"], respZ=r["respZ"], rtMsq=r["rtMsq"], rtZ=r["rtZ"], nObs=r["nObs"], nRows=r["nRows"], nNodes=r["nNodes"],
                         nCoarse=r["nCoarse"], nSubj=r["nSubj"])


def getItemFit(MCMC: _GibbsBase, nodes=_lib.MARGINAL_NODES) -> OutputItemFit:
    """Item fit of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- computed on the device from the resident item trace and data
    set (erm_get_item_fit / erm_farm_get_item_fit), in either trace mode: infit, outfit, respZ, rtMsq, rtZ, nObs per item.  On the calibration sample itself a
    misfit that a free a_j or sig2t_j absorbs does not show: check a second sample with itemFit.  nodes: as getWaicMarginal's."""
    Q = _marginal_check(MCMC, nodes, "getItemFit")
    return _item_fit_output(_marginal_source(MCMC, "getItemFit").item_fit(Q))


def itemFit(model, Y, logT, X, rows, nodes=_lib.MARGINAL_NODES, device=0, obs=None) -> OutputItemFit:
    """Item fit and drift of a sample -- a new one, or one that is no longer resident -- against saved item-trace rows [R, item_trace_width]
    (Engine.item_trace()), on the device (erm_item_fit); the arguments are scoreRespondents' without the weighting (the rows count equally).  respZ below -3: the
    item is harder for this sample than calibrated; rtZ above 3: slower.  obs [N, J], 0/1: respondents who did not see every item -- an item's sums run over the
    respondents that saw it, nObs counts them, an item nobody saw gets NaN."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("itemFit serves the five models without quantile weights")
    Y, logT = _masked_data(Y, logT, obs)
    return _item_fit_output(_lib.item_fit(model, Y, logT, X, rows, nodes=_lib.marginal_nodes(nodes), device=device, obs=obs))


# ------------------------------------------------------------------------------------------------------------------
# Plausible values (include/ertirt.h: erm_get_plausible_values).  K draws of every subject's (theta, zeta) from its posterior given the item-level
# trace: draw k reads row r_k, picks a node of the marginal WAIC's rule by Gumbel-max on Philox stream 16, spreads theta over the node's cell and shrinks it back to
# the row's mean and variance, and draws zeta from its Gaussian conditional.
# ------------------------------------------------------------------------------------------------------------------
def _pv_output(r) -> OutputPv:
    return OutputPv(theta=r["theta"], zeta=r["zeta"], node=r["node"], coarse=r["coarse"], nRows=r["nRows"], nNodes=r["nNodes"], nCoarse=r["nCoarse"], seed=r["seed"],
                    nObs=r.get("nObs"))


def getPlausibleValues(MCMC: _GibbsBase, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES) -> OutputPv:
    """K plausible values per subject of the last sample! -- of one engine or of the chain farm of sample!(...; devices=) -- drawn on the device from the resident
    item trace and data set (erm_get_plausible_values / erm_farm_get_plausible_values), in either trace mode: theta, zeta (N, K), node, coarse.  Draws from the
    posterior getScores summarises: at every row a draw has the mean and the variance getScores reports there.  The same (K, seed, nodes) gives the same draws."""
    Q = _marginal_check(MCMC, nodes, "getPlausibleValues")
    K, seed = _lib.pv_draws(K), _lib.pv_seed(seed)
    return _pv_output(_marginal_source(MCMC, "getPlausibleValues").plausible_values(K, seed, Q))


def drawPlausibleValues(model, Y, logT, X, rows, K=_lib.PV_DRAWS, seed=_lib.PV_SEED, nodes=_lib.MARGINAL_NODES, device=0, obs=None) -> OutputPv:
    """Plausible values of respondents -- new ones, or those of a run that is no longer resident -- against saved item-trace rows [R, item_trace_width]
    (Engine.item_trace()), on the device (erm_plausible_values).  model: the model code (_lib.MODEL_*); Y, logT [N, J], X [N, F] or None; every row counts once.
    obs [N, J], 0/1: respondents who did not see every item (erm_plausible_values_masked), as scoreRespondents takes it; the result carries nObs.
    nodes: as getWaicMarginal's -- the default of 61 flags every respondent of a form of several hundred items (the draws then sit on one or two nodes); raise it
    until nCoarse is 0 (255 at 896 items)."""
    if model not in _lib.MARGINAL_MODELS:
        raise ValueError("drawPlausibleValues serves the five models without quantile weights")
    Q, K, seed = _lib.marginal_nodes(nodes), _lib.pv_draws(K), _lib.pv_seed(seed)
    Y, logT = _masked_data(Y, logT, obs)
    return _pv_output(_lib.plausible_values(model, Y, logT, X, rows, K=K, seed=seed, nodes=Q, device=device, obs=obs))


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

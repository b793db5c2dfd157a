"""Config + data/parameter containers mirroring /root/reference/src/Base.pl.jl:45-136.

Field names follow the reference; Julia identifiers that are not valid Python (σ²t) get ASCII names, and every
field is also reachable under its Julia spelling through attribute aliases (Para.θ, Para.Σp, getattr(Para, "σ²t")).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class SimConditions:
    """src/Base.pl.jl:45-56"""
    nSubj: int
    nItem: int
    nFeat: int
    nIter: int
    nChain: int
    nBurnin: int
    nThin: int
    nRep: int
    qRa: float
    qRt: float


def setCond(*, nSubj=2000, nItem=15, nFeat=3, nIter=5000, nChain=4, nBurnin=None, nThin=1, nRep=10, qRa=0.5, qRt=0.5):
    """src/Base.pl.jl:59-62.  As in the reference the nBurnin kwarg is ignored and forced to round(nIter/2)
    (Julia's round: half to even, which Python's round() also implements)."""
    nBurnin = int(round(nIter / 2))
    return SimConditions(int(nSubj), int(nItem), int(nFeat), int(nIter), int(nChain), nBurnin, int(nThin), int(nRep),
                         float(qRa), float(qRt))


class InputData:
    """src/Base.pl.jl:67-78: computes kappa = Y .- 0.5 and logT = log.(T)."""

    def __init__(self, *, Y=(), T=(), X=()):
        self.Y = np.asarray(Y)
        self.κ = self.Y.astype(np.float64) - 0.5 if self.Y.size else np.zeros(0)
        self.T = np.asarray(T, dtype=np.float64)
        self.logT = np.log(self.T) if self.T.size else np.zeros(0)
        self.X = np.asarray(X, dtype=np.float64)

    kappa = property(lambda self: self.κ)


class InputData4R:
    """src/Base.pl.jl:86-95 (all fields given explicitly)."""

    def __init__(self, *, Y=(), κ=(), T=(), logT=(), X=(), kappa=None):
        self.Y = np.asarray(Y)
        self.κ = np.asarray(κ if kappa is None else kappa, dtype=np.float64)
        self.T = np.asarray(T, dtype=np.float64)
        self.logT = np.asarray(logT, dtype=np.float64)
        self.X = np.asarray(X, dtype=np.float64)

    kappa = property(lambda self: self.κ)


_ALIASES = {"ω": "omega", "θ": "theta", "ζ": "zeta", "λ": "lam", "σ²t": "sig2t", "σ2t": "sig2t", "ν": "nu", "β": "beta",
            "ρ": "rho", "Σp": "Sigp", "lambda_": "lam"}


class InputPara:
    """src/Base.pl.jl:100-115: mutable bag ω θ a b ζ λ σ²t ν β ρ Σp (ASCII: omega theta a b zeta lam sig2t nu beta rho Sigp)."""
    _fields = ("omega", "theta", "a", "b", "zeta", "lam", "sig2t", "nu", "beta", "rho", "Sigp")

    def __init__(self, **kw):
        for f in self._fields:
            object.__setattr__(self, f, np.zeros(0))
        for k, v in kw.items():
            setattr(self, k, v)

    def __setattr__(self, k, v):
        k = _ALIASES.get(k, k)
        if k not in self._fields:
            raise AttributeError(f"InputPara has no field {k}")
        object.__setattr__(self, k, np.asarray(v, dtype=np.float64))

    def __getattr__(self, k):
        if k in _ALIASES:
            return object.__getattribute__(self, _ALIASES[k])
        raise AttributeError(k)

    def __repr__(self):
        return "InputPara(" + ", ".join(f"{f}{tuple(getattr(self, f).shape)}" for f in self._fields if getattr(self, f).size) + ")"


class OutputDic:
    """src/Base.pl.jl:130-136"""

    def __init__(self, pD=None, DIC=None):
        self.pD = pD
        self.DIC = DIC

    def __repr__(self):
        return f"OutputDic(pD={self.pD}, DIC={self.DIC})"


class OutputWaic:
    """WAIC of a fit (getWaic; the reference offers DIC only): elpd = sum_u (lppd_u - p_u), pWaic = sum_u p_u, WAIC = -2 elpd, se = 2 sqrt(U Var_u(elpd_u)),
    nHighVar = number of units with p_u > 0.4; unit is "subject" or "cell", nUnits = U, nRows = the post-burn-in rows behind it.  lppd_u / p_u (pointwise=True):
    subjects in order, cells as (nSubj, nItem).  unit "subject-marginal" (getWaicMarginal): theta_i and zeta_i integrated out; nNodes = the nodes of the theta
    rule, nCoarse = the subjects whose posterior was too narrow for it at some row (None for the conditional WAIC)."""

    def __init__(self, elpd=None, pWaic=None, WAIC=None, se=None, nHighVar=None, lppd=None, unit=None, nUnits=None, nRows=None, lppd_u=None, p_u=None,
                 nNodes=None, nCoarse=None):
        self.elpd, self.pWaic, self.WAIC, self.se, self.nHighVar = elpd, pWaic, WAIC, se, nHighVar
        self.lppd, self.unit, self.nUnits, self.nRows = lppd, unit, nUnits, nRows
        self.lppd_u, self.p_u = lppd_u, p_u
        self.nNodes, self.nCoarse = nNodes, nCoarse

    @property
    def elpd_u(self):
        return None if self.lppd_u is None else self.lppd_u - self.p_u

    def __repr__(self):
        return f"OutputWaic(unit={self.unit!r}, elpd={self.elpd}, pWaic={self.pWaic}, WAIC={self.WAIC}, se={self.se}, nHighVar={self.nHighVar})"


class OutputLoo:
    """Marginal PSIS-LOO of a fit (getLooMarginal / psisLoo; the reference offers DIC only): elpd = sum_u elpd_u, pLoo = sum_u p_u, LOOIC = -2 elpd,
    se = 2 sqrt(U Var_u(elpd_u)), lppd; nBadK = the units with khat > 0.7 (Inf included), nHighK = those above the sample-size dependent threshold
    min(1 - 1 / log10(nRows), 0.7); tailLen = M, the values the generalised Pareto law is fitted to; nNodes, nCoarse as OutputWaic's.  Pointwise (subjects in
    order): elpd_u, p_u, khat (the Pareto shape of the subject's importance ratios: above the threshold the posterior would move if the subject were left out --
    an aberrant or influential respondent -- and elpd_u is optimistic; +Inf: the tail could not be fitted), nEff (the effective number of rows behind elpd_u)."""

    def __init__(self, elpd=None, pLoo=None, LOOIC=None, se=None, lppd=None, unit=None, nUnits=None, nRows=None, nBadK=None, nHighK=None, tailLen=None,
                 elpd_u=None, p_u=None, khat=None, nEff=None, nNodes=None, nCoarse=None):
        self.elpd, self.pLoo, self.LOOIC, self.se, self.lppd = elpd, pLoo, LOOIC, se, lppd
        self.unit, self.nUnits, self.nRows, self.nBadK, self.nHighK, self.tailLen = unit, nUnits, nRows, nBadK, nHighK, tailLen
        self.elpd_u, self.p_u, self.khat, self.nEff = elpd_u, p_u, khat, nEff
        self.nNodes, self.nCoarse = nNodes, nCoarse

    @property
    def lppd_u(self):
        return None if self.elpd_u is None else self.elpd_u + self.p_u

    def __repr__(self):
        return f"OutputLoo(unit={self.unit!r}, elpd={self.elpd}, pLoo={self.pLoo}, LOOIC={self.LOOIC}, se={self.se}, nBadK={self.nBadK}, nHighK={self.nHighK})"


class OutputScores:
    """Scores of the respondents (getScores / scoreRespondents; the reference has no counterpart): per subject theta, thetaSd (the posterior mean of ability and its
    standard error), zeta, zetaSd, cov (of theta and zeta; the three are NaN for GibbsMlIrt), rowEss (the rows' effective size: nRows under equal weights) and
    coarse (the theta rule was too coarse for the subject at some row: raise nodes); nRows, nNodes, nCoarse.  relTheta / relZeta: the EAP reliability
    Var_i(score_i) / (Var_i(score_i) + mean_i sd_i^2)."""

    def __init__(self, theta=None, thetaSd=None, zeta=None, zetaSd=None, cov=None, rowEss=None, coarse=None, nRows=None, nNodes=None, nCoarse=None, weighting="equal", nObs=None):
        self.theta, self.thetaSd, self.zeta, self.zetaSd, self.cov, self.rowEss, self.coarse = theta, thetaSd, zeta, zetaSd, cov, rowEss, coarse
        self.nRows, self.nNodes, self.nCoarse, self.weighting = nRows, nNodes, nCoarse, weighting
        self.nObs = nObs          # scoreRespondents(..., obs=): the observed cells per subject (None without a mask)

    @staticmethod
    def _rel(m, sd):
        if m is None or np.any(np.isnan(m)):
            return float("nan")
        between = float(np.var(m))
        return between / (between + float(np.mean(np.square(sd))))

    @property
    def relTheta(self):
        return self._rel(self.theta, self.thetaSd)

    @property
    def relZeta(self):
        return self._rel(self.zeta, self.zetaSd)

    def __repr__(self):
        return (f"OutputScores(nSubj={None if self.theta is None else np.size(self.theta)}, nRows={self.nRows}, nNodes={self.nNodes}, nCoarse={self.nCoarse}, "
                f"relTheta={self.relTheta:.4f}, relZeta={self.relZeta:.4f})")


class OutputPersonFit:
    """Person fit of the respondents (getPersonFit / personFit; the reference has no counterpart): per subject lz (Drasgow, Levine and Williams' standardised
    log-likelihood of the responses, averaged over the posterior of theta; negative: misfit) with pResp, its posterior predictive p-value under lz's normal
    approximation; ltz (the Wilson-Hilferty z of the response-time quadratic form; positive: misfit) with pTime, its exact chi^2 posterior predictive p-value
    (both NaN for GibbsMlIrt); small p-values mean misfit.  rowEss, coarse, nRows, nNodes, nCoarse as OutputScores'; nObs: the observed cells per subject (None
    without a mask).  A subject without an observed cell has NaN in the four statistics."""

    def __init__(self, lz=None, pResp=None, ltz=None, pTime=None, rowEss=None, coarse=None, nRows=None, nNodes=None, nCoarse=None, weighting="equal", nObs=None):
        self.lz, self.pResp, self.ltz, self.pTime, self.rowEss, self.coarse = lz, pResp, ltz, pTime, rowEss, coarse
        self.nRows, self.nNodes, self.nCoarse, self.weighting, self.nObs = nRows, nNodes, nCoarse, weighting, nObs

    def flagged(self, alpha=0.05):
        """(responses, times): boolean (N,) -- the p-value is below alpha (NaN is not flagged)."""
        below = lambda p: np.zeros(0, dtype=bool) if p is None else np.nan_to_num(np.asarray(p, dtype=np.float64), nan=1.0) < alpha
        return below(self.pResp), below(self.pTime)

    def __repr__(self):
        fr, ft = self.flagged()
        return (f"OutputPersonFit(nSubj={None if self.lz is None else np.size(self.lz)}, nRows={self.nRows}, nNodes={self.nNodes}, nCoarse={self.nCoarse}, "
                f"flaggedResp={int(np.sum(fr))}, flaggedTime={int(np.sum(ft))})")


class OutputItemFit:
    """Item fit and drift (getItemFit / itemFit; the reference has no counterpart): per item infit and outfit (mean squares of the response residuals, about 1),
    respZ (the signed response residual; negative: harder than calibrated), rtMsq (mean square of the leave-one-item-out response-time residual, about 1) and rtZ
    (its signed sum; positive: slower than calibrated) -- the two time columns NaN for GibbsMlIrt --, nObs (J,) the subjects that observed the item (an item nobody
    observed has NaN in the five statistics); nSubj, nRows, nNodes, nCoarse as OutputScores'.  The signed columns are the ones that find drift in a new sample; a
    misfit that a free a_j or sig2t_j absorbs does not show on the item's own calibration sample."""

    def __init__(self, infit=None, outfit=None, respZ=None, rtMsq=None, rtZ=None, nObs=None, nRows=None, nNodes=None, nCoarse=None, nSubj=None):
        self.infit, self.outfit, self.respZ, self.rtMsq, self.rtZ, self.nObs = infit, outfit, respZ, rtMsq, rtZ, nObs
        self.nRows, self.nNodes, self.nCoarse, self.nSubj = nRows, nNodes, nCoarse, nSubj

    def flagged(self, z=3.0, lo=0.7, hi=1.3):
        """(responses, times): boolean (J,) -- |respZ| (|rtZ|) is at least z, or infit (rtMsq) lies outside [lo, hi]; NaN is not flagged."""
        def flag(sz, msq):
            if sz is None or msq is None:
                return np.zeros(0, dtype=bool)
            sz, msq = np.asarray(sz, dtype=np.float64), np.asarray(msq, dtype=np.float64)
            with np.errstate(invalid="ignore"):
                return (np.abs(sz) >= z) | (msq < lo) | (msq > hi)
        return flag(self.respZ, self.infit), flag(self.rtZ, self.rtMsq)

    def __repr__(self):
        fr, ft = self.flagged()
        return (f"OutputItemFit(nItem={None if self.infit is None else np.size(self.infit)}, nSubj={self.nSubj}, nRows={self.nRows}, nNodes={self.nNodes}, "
                f"nCoarse={self.nCoarse}, flaggedResp={int(np.sum(fr))}, flaggedTime={int(np.sum(ft))})")


class OutputPv:
    """Plausible values of the respondents (getPlausibleValues / drawPlausibleValues; the reference has no counterpart): theta (N, K) and zeta (N, K), K draws per
    subject from its posterior given the item trace (zeta is NaN for GibbsMlIrt); node (N, K), the rule's node behind every draw; coarse (N,), the theta rule was too
    coarse for the subject at some row it used (raise nodes); nRows, nNodes, nCoarse and the seed of the draws.  Column k over the subjects is one imputed data set:
    analyse each of the K and pool the results by Rubin's rules."""

    def __init__(self, theta=None, zeta=None, node=None, coarse=None, nRows=None, nNodes=None, nCoarse=None, seed=None, nObs=None):
        self.theta, self.zeta, self.node, self.coarse = theta, zeta, node, coarse
        self.nRows, self.nNodes, self.nCoarse, self.seed = nRows, nNodes, nCoarse, seed
        self.nObs = nObs          # drawPlausibleValues(..., obs=): the observed cells per subject (None without a mask)

    def __repr__(self):
        shape = None if self.theta is None else np.shape(self.theta)
        return f"OutputPv(shape={shape}, nRows={self.nRows}, nNodes={self.nNodes}, nCoarse={self.nCoarse}, seed={self.seed})"


class OutputPpc:
    """Posterior predictive checks of a fit (getPpc / getPpcHost; the reference has no counterpart).  R = the number of replicated data sets; item (3, 4, nItem),
    subj (2, 4, nSubj), total (2, 4): components RA (response deviance), RT (response-time chi^2; NaN for GibbsMlIrt)[, SCORE (item score)] x
    {n_ge = #(rep >= obs), n_gt = #(rep > obs), mean of obs, mean of rep}.  ppp(...) = n_ge / R, ppp_mid(...) = (n_gt + (n_ge - n_gt) / 2) / R."""

    COMPONENTS = {"ra": 0, "rt": 1, "score": 2}

    def __init__(self, R=None, thin=None, item=None, subj=None, total=None):
        self.R, self.thin, self.item, self.subj, self.total = R, thin, item, subj, total

    def _pick(self, unit, comp):
        a = {"item": self.item, "subject": self.subj, "total": self.total}[unit]
        c = self.COMPONENTS[comp]
        if c >= a.shape[0]:
            raise ValueError("the item score is a test quantity of the items only")
        return a[c]

    def ppp(self, unit="item", comp="ra"):
        return self._pick(unit, comp)[0] / self.R

    def ppp_mid(self, unit="item", comp="ra"):
        a = self._pick(unit, comp)
        return (a[1] + 0.5 * (a[0] - a[1])) / self.R

    def mean_obs(self, unit="item", comp="ra"):
        return self._pick(unit, comp)[2]

    def mean_rep(self, unit="item", comp="ra"):
        return self._pick(unit, comp)[3]

    def __repr__(self):
        return f"OutputPpc(R={self.R}, thin={self.thin}, total ppp RA={self.ppp('total', 'ra')}, RT={self.ppp('total', 'rt')})"

"""The refusals of the marginal getters, word for word and without a device: every sampler class against getWaicMarginal, getLooMarginal, getScores,
getPlausibleValues, getWaicMarginalQr, getLooMarginalQr and the two host WAIC variants -- a model the family does not serve, the wrong family, a subject-sharded
sampler, a bad node count, too few rows for PSIS-LOO, no data for a host variant, and a sampler that has not run.  The texts are those of the front end before
the two families shared one check; {cls} stands for the sampler's class name."""
import numpy as np
import pytest

import parity_util as pu

GAUSSIAN = ("GibbsMlIrt", "GibbsRtIrt", "GibbsRtIrtNull", "GibbsRtIrtCross", "GibbsRtIrtLatent")
QUANTILE = ("GibbsRtIrtLatentQr",)
CLASSES = GAUSSIAN + QUANTILE + ("GibbsRtIrtCrossQr",)

NODES = "nodes must be odd and in 3 .. 1025"
FEW_ROWS = "PSIS-LOO needs 25 .. 8192 rows per unit (4 given)"
NO_DATA = "Data is required"
# getter -> (the classes it serves, its texts)
GETTERS = {
    "getWaicMarginal": (GAUSSIAN, dict(
        unserved="getWaicMarginal is not available for {cls}: with the quantile weights integrated out the response-time term is not Gaussian in zeta "
                 "(GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)",
        sharded="getWaicMarginal is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getWaicMarginal reads the engine's resident item trace and data set)")),
    "getLooMarginal": (GAUSSIAN, dict(
        unserved="getLooMarginal is not available for {cls}: with the quantile weights integrated out the response-time term is not Gaussian in zeta "
                 "(GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)",
        sharded="getLooMarginal is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getLooMarginal reads the engine's resident item trace and data set)")),
    "getScores": (GAUSSIAN, dict(
        unserved="getScores is not available for {cls}: with the quantile weights integrated out the response-time term is not Gaussian in zeta "
                 "(GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)",
        sharded="getScores is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getScores reads the engine's resident item trace and data set)")),
    "getPlausibleValues": (GAUSSIAN, dict(
        unserved="getPlausibleValues is not available for {cls}: with the quantile weights integrated out the response-time term is not Gaussian in zeta "
                 "(GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)",
        sharded="getPlausibleValues is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getPlausibleValues reads the engine's resident item trace and data set)")),
    "getWaicMarginalQr": (QUANTILE, dict(
        wrong_family="getWaicMarginalQr is for GibbsRtIrtLatentQr: {cls} has no quantile weights, use getWaicMarginal",
        unserved="getWaicMarginalQr is not available for {cls}: with the quantile weights nu_ij integrated out every cell's response time is asymmetric Laplace in "
                 "zeta, and the zeta integral (J kinks that move with theta) has no closed form",
        sharded="getWaicMarginalQr is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getWaicMarginalQr reads the engine's resident item trace and data set)")),
    "getLooMarginalQr": (QUANTILE, dict(
        wrong_family="getLooMarginalQr is for GibbsRtIrtLatentQr: {cls} has no quantile weights, use getLooMarginal",
        unserved="getLooMarginalQr is not available for {cls}: with the quantile weights nu_ij integrated out every cell's response time is asymmetric Laplace in "
                 "zeta, and the zeta integral (J kinks that move with theta) has no closed form",
        sharded="getLooMarginalQr is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getLooMarginalQr reads the engine's resident item trace and data set)")),
    # the host variants refuse in the device getter's name, and fetch their rows through marginalRows, which asks in getWaicMarginal's
    "getWaicMarginalHost": (GAUSSIAN, dict(
        unserved="getWaicMarginal is not available for {cls}: with the quantile weights integrated out the response-time term is not Gaussian in zeta "
                 "(GibbsRtIrtLatentQr: getWaicMarginalQr / getLooMarginalQr; GibbsRtIrtCrossQr: the zeta integral has no closed form)",
        sharded="getWaicMarginal is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getWaicMarginal reads the engine's resident item trace and data set)")),
    "getWaicMarginalQrHost": (QUANTILE, dict(
        wrong_family="getWaicMarginalQr is for GibbsRtIrtLatentQr: {cls} has no quantile weights, use getWaicMarginal",
        unserved="getWaicMarginalQr is not available for {cls}: with the quantile weights nu_ij integrated out every cell's response time is asymmetric Laplace in "
                 "zeta, and the zeta integral (J kinks that move with theta) has no closed form",
        sharded="getWaicMarginalQr is not available for a subject-sharded sampler (every subject's data must be resident on one device)",
        unrun="run sample! first (getWaicMarginal reads the engine's resident item trace and data set)")),
}


def _sampler(pkg, cls, *, n_iter=60, shard=False, data=True):
    """A sampler on toy data that never meets an engine; nIter = 60 leaves 30 post-burn-in rows, enough for PSIS-LOO."""
    N, J, F = 6, 3, 2
    g = np.random.default_rng(1)
    D = pkg.InputData(Y=g.integers(0, 2, (N, J)), T=np.exp(g.standard_normal((N, J))), X=g.standard_normal((N, F))) if data else None
    M = getattr(pkg, cls)(pkg.setCond(nSubj=N, nItem=J, nFeat=F, nIter=n_iter, nChain=1), Data=D, shard=(0, 1, N, 0, b"\0" * 128) if shard else None)
    assert M._engine is None and M.farm is None
    return M


def _text(fn, M, **kw):
    with pytest.raises(ValueError) as e:
        fn(M, **kw)
    return str(e.value)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("getter", GETTERS)
def test_refusal_texts_are_the_literal_strings(getter, cls):
    pkg = pu.ge.load_package()
    fn, (served, texts) = getattr(pkg, getter), GETTERS[getter]
    if cls not in served:
        want = texts["wrong_family" if served == QUANTILE and cls in GAUSSIAN else "unserved"].format(cls=cls)
        for kw in (dict(), dict(shard=True), dict(n_iter=8), dict(data=False)):          # the model is refused before anything else is looked at
            assert _text(fn, _sampler(pkg, cls, **kw)) == want, kw
        assert _text(fn, _sampler(pkg, cls), nodes=60) == want
        return
    assert _text(fn, _sampler(pkg, cls, shard=True)) == texts["sharded"]
    assert _text(fn, _sampler(pkg, cls, shard=True), nodes=60) == texts["sharded"]
    for bad in (60, 1, 1027, 4.5):
        assert _text(fn, _sampler(pkg, cls), nodes=bad) == NODES, bad
    if "Loo" in getter:
        assert _text(fn, _sampler(pkg, cls, n_iter=8)) == FEW_ROWS
        assert _text(fn, _sampler(pkg, cls, n_iter=8), nodes=60) == NODES
    if getter.endswith("Host"):
        assert _text(fn, _sampler(pkg, cls, data=False)) == NO_DATA
    assert _text(fn, _sampler(pkg, cls)) == texts["unrun"]

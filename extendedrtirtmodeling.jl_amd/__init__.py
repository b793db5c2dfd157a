"""MI355X-native Gibbs engine for the `sample!` hot path of ExtendedRtIrtModeling.jl.

Export list mirrors the part of /root/reference/src/ExtendedRtIrtModeling.jl:33-77 that belongs to the hot path.
"""
from .base import InputData, InputData4R, InputPara, OutputDic, OutputItemFit, OutputLoo, OutputPersonFit, OutputPpc, OutputPv, OutputScores, OutputWaic, SimConditions, setCond
from .gibbs import (GibbsMlIrt, GibbsRtIrt, GibbsRtIrtCross, GibbsRtIrtCrossQr, GibbsRtIrtLatent, GibbsRtIrtLatentQr, GibbsRtIrtNull,
                    GibbsRtIrtQuantile, checkConvergence, coef, compareLoo, compareWaic, drawPlausibleValues, getDic, getDicHost, getLogLikelihood,
                    getItemFit, getLooMarginal, getLooMarginalQr, getPersonFit, getPlausibleValues, getPpc, getScores, getWaic, getWaicMarginal, getWaicMarginalQr, itemFit, observedMask, personFit, precis, psisLoo,
                    sample, sample_b, scoreRespondents, simulateData)
from .twins import (ess_rhat, getLooMarginalHost, getLooMarginalQrHost, getPpcHost, getWaicHost, getWaicMarginalHost, getWaicMarginalQrHost,
                    itemFitHost, marginalLogLikHost, personFitHost, plausibleValuesHost, pointwiseLogLikHost, psisLooHost, quantileMarginalLogLikHost, rank_ess_rhat, scoresHost)
from .simtools import (comparePara, getBias, getMetrics, getMetrics2, getRmse, runSimulation, setDataMlIrt, setDataRtIrt, setDataRtIrtCross,
                       setDataRtIrtLatent, setDataRtIrtNull,
                       setTrueParaMlIrt, setTrueParaRtIrt, setTrueParaRtIrtCross, setTrueParaRtIrtLatent)
from . import _lib, gibbs, parallel, twins

# The twins that callers reached as attributes of the gibbs module without their being exported here keep that address (gibbs.py itself reads nothing from
# twins.py: the names are set from outside, once both modules are loaded).
for _name in ("ess_rhat", "rank_ess_rhat", "waicFromLogLik", "psisTailLen", "pvRow", "pvGumbel", "pvFinish", "_philox4x32_10", "_ppc_uniform", "_ppc_normal",
              "_ppc_stream_word3"):
    setattr(gibbs, _name, getattr(twins, _name))
del _name

__all__ = [
    "setCond", "SimConditions", "InputData", "InputData4R", "InputPara", "OutputDic",
    "setDataMlIrt", "setDataRtIrt", "setDataRtIrtCross", "setDataRtIrtLatent", "setDataRtIrtNull", "runSimulation", "getMetrics", "getMetrics2",
    "comparePara",
    "setTrueParaMlIrt", "setTrueParaRtIrt", "setTrueParaRtIrtCross", "setTrueParaRtIrtLatent",
    "getBias", "getRmse", "getDic", "getDicHost", "getWaic", "getWaicHost", "compareWaic", "pointwiseLogLikHost",
    "getWaicMarginal", "getWaicMarginalHost", "marginalLogLikHost", "OutputWaic", "getScores", "scoreRespondents", "scoresHost", "OutputScores",
    "getPersonFit", "personFit", "personFitHost", "OutputPersonFit",
    "getItemFit", "itemFit", "itemFitHost", "OutputItemFit",
    "getPlausibleValues", "drawPlausibleValues", "plausibleValuesHost", "OutputPv", "observedMask", "getLooMarginal", "getLooMarginalHost",
    "getWaicMarginalQr", "getWaicMarginalQrHost", "getLooMarginalQr", "getLooMarginalQrHost", "quantileMarginalLogLikHost",
    "psisLoo", "psisLooHost", "compareLoo", "OutputLoo", "getPpc", "getPpcHost", "OutputPpc", "checkConvergence", "ess_rhat", "rank_ess_rhat",
    "simulateData", "getLogLikelihood", "sample_b", "sample",
    "GibbsMlIrt", "GibbsRtIrt", "GibbsRtIrtCrossQr", "GibbsRtIrtLatentQr", "GibbsRtIrtQuantile", "GibbsRtIrtNull", "GibbsRtIrtCross", "GibbsRtIrtLatent", "coef", "precis",
]

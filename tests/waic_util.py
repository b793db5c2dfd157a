"""Helpers shared by the WAIC tests (tests/test_waic_host.py, tests/test_gpu_waic.py): a sampler-shaped namespace around trace arrays for getWaicHost, and the
data set of the 2pl-against-1pl comparison."""
import types

import numpy as np

import parity_util as pu

MODEL_CODE = {"mlirt": 0, "rtirt": 1, "crossqr": 2, "latentqr": 3, "null": 4, "cross": 5, "latent": 6}


def as_sampler(model, Y, logT, ra, rt, qr, *, nIter, nChain, nBurnin, qRt=0.85):
    """What getWaicHost reads of a sampler: Cond, Data, Post.ra / rt / qr in Julia layout (nIter, width, nChain), _model."""
    N, J = Y.shape
    Cond = types.SimpleNamespace(nSubj=N, nItem=J, nIter=nIter, nChain=nChain, nBurnin=nBurnin, qRt=qRt)
    Data = types.SimpleNamespace(Y=Y, logT=logT)
    Post = types.SimpleNamespace(ra=ra, rt=rt, qr=qr)
    return types.SimpleNamespace(Cond=Cond, Data=Data, Post=Post, _model=MODEL_CODE[model], farm=None)


def rows_to_julia(rows, nChain=1):
    """(rows, width) with row = m * nChain + l  ->  (nIter, width, nChain)."""
    r, w = rows.shape
    return np.asfortranarray(rows.reshape(r // nChain, nChain, w).transpose(0, 2, 1))


def oracle_sampler(model, Y, logT, X, init, nsweeps, *, qRt=0.85, onepl=False, nBurnin=None, seed=1234):
    """An oracle chain of nsweeps rows (one chain) wrapped for getWaicHost."""
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=qRt, onepl=onepl, cov2one=model not in ("latentqr", "latent"), seed=seed)
    t = op.run(nsweeps, with_nu=model in ("latentqr", "crossqr"))
    return as_sampler(model, Y, logT, rows_to_julia(t["ra"]), rows_to_julia(t["rt"]), rows_to_julia(t["qr"]), nIter=nsweeps, nChain=1,
                      nBurnin=nsweeps // 2 if nBurnin is None else nBurnin, qRt=qRt)


# the 2pl-against-1pl comparison: size and chain length fixed on the CPU with the oracle chain (tests/test_waic_host.py)
SPREAD_N, SPREAD_J, SPREAD_ITER = 600, 12, 200


def spread_problem(N=SPREAD_N, J=SPREAD_J, seed=5):
    """GibbsMlIrt data with widely spread discriminations (0.25 ... 3): a 1pl fit, one common slope, cannot follow them."""
    g = np.random.default_rng(seed)
    a = np.linspace(0.25, 3.0, J)
    b = g.uniform(-1.0, 1.0, J)
    X = g.standard_normal((N, 1))
    theta = 0.5 * X[:, 0] + g.standard_normal(N)
    pr = 1.0 / (1.0 + np.exp(-(a[None, :] * (theta[:, None] - b[None, :]))))
    Y = (g.uniform(size=(N, J)) < pr).astype(np.uint8)
    init = dict(theta=g.standard_normal(N), beta=g.standard_normal(2))
    return Y, X, init

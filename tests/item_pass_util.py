"""What the GPU tests of the item-trace passes (marginal WAIC, its quantile family, PSIS-LOO, scores, plausible values) share: the package, the covariates a
model's kernels see, an engine and a farm set up on a parity_util problem, and the bytes of an entry's result."""
import numpy as np

import parity_util as pu


def _pkg():
    return pu.ge.load_package()


def _kernel_x(model, X):
    return X if model in ("mlirt", "rtirt", "latent") else None


def _config(model, Y, X, n_iter, n_chain, n_burnin, precision, full, q_rt):
    N, J = Y.shape
    return dict(model=pu.MODELS[model], n_item=J, n_subj=N, n_feat=0 if X is None else X.shape[1], n_iter=n_iter, n_chain=n_chain, n_burnin=n_burnin,
                cov2one=int(model not in ("latentqr", "latent")), q_rt=q_rt, seed=1234, precision={"f32": 0, "f64": 1}[precision], trace_mode=int(full))


def _engine(model, Y, logT, X, init, *, n_iter, n_burnin, n_chain=1, precision="f64", full=True, unit=None, onepl=False, q_rt=0.85):
    eng = _pkg()._lib.Engine(one_pl=int(onepl), **_config(model, Y, X, n_iter, n_chain, n_burnin, precision, full, q_rt))
    eng.set_data(Y, logT, X)
    if unit is not None:
        eng.set_pointwise(unit)
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    return eng


def _farm(model, devices, Y, logT, X, init, *, n_iter, n_burnin, precision="f64", q_rt=0.85):
    """One chain per entry of devices, in summary mode; chain 0 starts from init, the others from their own theta and zeta."""
    farm = _pkg()._lib.Farm(devices, **_config(model, Y, X, n_iter, 1, n_burnin, precision, False, q_rt))
    farm.set_data(Y, logT, X)
    g = np.random.default_rng(3)
    for l in range(len(devices)):
        st = {("lambda_" if k == "lam" else k): (v if l == 0 or k not in ("theta", "zeta") else g.standard_normal(Y.shape[0])) for k, v in init.items()}
        farm.set_state(l, **st)
    return farm


def _bytes(r):
    """Every scalar (by repr) and every array (by its bytes) of an entry's result, keys in order: the dict of an entry, or the marginal WAIC's (totals, lppd, p)."""
    items = sorted((dict(r[0], lppd_i=r[1], p_i=r[2]) if isinstance(r, tuple) else r).items())
    return repr([(k, v) for k, v in items if not isinstance(v, np.ndarray)]).encode() + b"".join(np.ascontiguousarray(v).tobytes() for _, v in items if isinstance(v, np.ndarray))

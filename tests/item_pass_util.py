"""What the GPU tests of the item-trace passes (marginal WAIC, its quantile family, PSIS-LOO, scores, plausible values) share: the package, the covariates a
model's kernels see, an engine and a farm set up on a parity_util problem, and the bytes of an entry's result; and, for tests/test_item_pass_limits_host.py and
tests/test_gpu_item_pass_limits.py, the one table of limit cases (896 items, the two sides of the 64 KB line of dynamic LDS, 1025 nodes, 14 covariates)."""
import functools

import numpy as np

import marginal_util as mu
import obs_util as ou
import parity_util as pu
import pv_util as pvu
import qmarginal_util as qu


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


# ------------------------------------------------------------------------------------------------------------ the limit cases
# One table for tests/test_item_pass_limits_host.py (the preconditions, on the CPU with the twins alone) and tests/test_gpu_item_pass_limits.py (the kernels).
# A case is a tuple whose head names its kind:
#   ("wide", model, J)              N = 40 (one full tile of 32 and a tile with 24 idle subject slots), 3 rows, F = 3, Q = 255
#   ("masked", model)               obs_util.problem(model, 33, 896, 3, ...): n_i = 896, 0, 1, 888, 448 and about 448 side by side in one wave, Q = 255
#   ("nodes", model, Q)             J = 9, N = 37, 3 rows, F = 3
#   ("feat", model, masked)         J = 9, N = 37, 3 rows, F = 14, Q = 61; masked: with obs_util.masks
# model is one of marginal_util.MODELS or "latentqr" (the quantile entry at Q_RT).  problem(case) is the case's inputs, twin(case, product) its reference, each
# computed once per process and never written to.
J_MAX, Q_MAX, F_MAX = 896, 1025, 14          # what the entries accept: n_item, MARG_NODES_MAX, MARG_MAXF
LDS_LINE = 65536                             # dynamic LDS above this many bytes needs hipFuncAttributeMaxDynamicSharedMemorySize (marg_tile_launch)
COARSE_S, S_MARGIN = 2.0, 0.1                # MARG_COARSE_S, and how far every twin S of a case must stay from it for the flags to be decidable
Q_RT = 0.85
CODE = dict(mu.CODE, latentqr=qu.CODE)
WIDE_N, WIDE_Q, MASKED_N, SMALL_N, SMALL_J, ROWS, K_DRAWS, PV_SEED = 40, 255, 33, 37, 9, 3, 5, pvu.CASE_SEED
NODE_COUNTS = (63, 65, 513, 1025)            # 63 of the 64 slots of one lane chunk; one node on the second trip; lane 0 alone on the last trip after 8 and 16 full ones
X_MODELS = ("mlirt", "rtirt", "latent")      # the Gaussian models whose kernels see X
SEEDS = {}                                   # case -> data seed where DEFAULT_SEED fails a precondition of tests/test_item_pass_limits_host.py (none does)
DEFAULT_SEED = 7


def marg_lds_bytes(model, J, F):
    """The dynamic LDS of one launch of marginal_kernel, score_kernel or pv_kernel: marg_lds of csrc/erm_item_pass.hpp, two halves of marg_row_lds = the row and
    g_j, log sig2t_j beside it, in doubles."""
    return 16 * (_pkg()._lib.item_trace_width(CODE[model], J, F) + 2 * J)


def lds_straddle(model, F):
    """(J_lo, J_hi): the largest item count whose launch asks for at most LDS_LINE bytes, and the next one."""
    J_lo = max(J for J in range(1, J_MAX) if marg_lds_bytes(model, J, F) <= LDS_LINE)
    return J_lo, J_lo + 1


def products(model):
    """The products of section 3 a model has: marginal_loglik, score (both weightings) and plausible_values, or LatentQr's quantile_marginal_loglik."""
    return ("qloglik",) if model == "latentqr" else ("loglik", "score", "pv")


WIDE_CASES = [("wide", m, J_MAX) for m in mu.MODELS + ["latentqr"]] + [("wide", m, J) for m in ("cross", "rtirt") for J in lds_straddle(m, 3)]
MASKED_CASES = [("masked", m) for m in ("rtirt", "cross", "mlirt")]
NODE_CASES = [("nodes", m, Q) for Q in NODE_COUNTS for m in mu.MODELS + ["latentqr"]]
FEAT_CASES = [("feat", m, masked) for m in X_MODELS for masked in (False, True)] + [("feat", "latentqr", False)]


def case_id(case):
    return "-".join("masked" if v is True else "complete" if v is False else str(v) for v in case)


class Problem:
    """The inputs of a case: model (the name), code, Y, logT, X (as the kernels see it), rows, obs (None: complete), Q, and K, seed for the draws."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        for a in (self.Y, self.logT, self.X, self.rows, self.obs):
            if a is not None:
                a.setflags(write=False)

    @property
    def data(self):
        return self.Y, self.logT, self.X


@functools.lru_cache(maxsize=None)
def problem(case):
    kind, model = case[0], case[1]
    seed = SEEDS.get(case, DEFAULT_SEED)
    N, J, F, Q, masked = {"wide": lambda: (WIDE_N, case[2], 3, WIDE_Q, False), "masked": lambda: (MASKED_N, J_MAX, 3, WIDE_Q, True),
                          "nodes": lambda: (SMALL_N, SMALL_J, 3, case[2], False), "feat": lambda: (SMALL_N, SMALL_J, F_MAX, 61, case[2])}[kind]()
    obs = None
    if model == "latentqr":
        rows, (Y, logT, X) = qu.make_rows(J, F, ROWS, seed=seed), qu.make_data(N, J, F, seed=seed)
    elif masked:
        Y, logT, X, rows, obs = ou.problem(model, N, J, ROWS, seed=seed, F=F)
    else:
        Y, logT, X, rows = pvu.problem(model, N, J, F, ROWS, seed=seed)
    return Problem(model=model, code=CODE[model], Y=Y, logT=logT, X=X, rows=rows, obs=obs, Q=Q, K=K_DRAWS, seed=PV_SEED)


def twin_of(p, product):
    """The numpy twin of a product on the inputs p (a Problem): "loglik" and "qloglik" -> (l (R, N), S (R, N)); "score.equal", "score.likelihood" -> OutputScores;
    "pv" -> (OutputPv, gap (N, K))."""
    pkg = _pkg()
    kw = {} if p.obs is None else dict(obs=p.obs)
    if product == "loglik":
        return pkg.marginalLogLikHost(p.code, *p.data, p.rows, p.Q, with_S=True, **kw)
    if product == "qloglik":
        return pkg.quantileMarginalLogLikHost(p.code, *p.data, p.rows, Q_RT, p.Q, with_S=True)
    if product.startswith("score."):
        return pkg.scoresHost(p.code, *p.data, p.rows, p.Q, product[6:], **kw)
    if product == "pv":
        return pkg.plausibleValuesHost(p.code, *p.data, p.rows, p.K, p.seed, p.Q, with_gap=True, **kw)
    raise ValueError(product)


@functools.lru_cache(maxsize=None)
def twin(case, product):
    return twin_of(problem(case), product)


def twin_keys(cases):
    """Every (case, product) whose twin the two test files read: the score under both weightings."""
    return [(c, k) for c in cases for pr in products(c[1]) for k in (("score.equal", "score.likelihood") if pr == "score" else (pr,))]


def warm_twins(cases, workers=8):
    """Fills twin()'s cache for the cases on a few threads (numpy releases the interpreter lock inside its loops over the (N, Q, J) arrays), so that a module's
    references cost seconds, not a minute; the values are those a lone call gives."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(lambda k: twin(*k), twin_keys(cases)))


def twins_of(p, keys, workers=8):
    """{key: twin_of(p, key)} on a few threads, for inputs that are no case of the table (an engine's chain)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return dict(zip(keys, ex.map(lambda k: twin_of(p, k), keys)))


def twin_loglik_by_rows(p, product="loglik", workers=8):
    """twin_of(p, "loglik") for a long table: the rows are independent of one another, so they go to the threads one at a time and every l and S is the lone call's."""
    from concurrent.futures import ThreadPoolExecutor
    one = lambda r: twin_of(Problem(**dict(p.__dict__, rows=p.rows[r:r + 1].copy())), product)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        parts = list(ex.map(one, range(p.rows.shape[0])))
    return np.concatenate([a for a, _ in parts], axis=0), np.concatenate([b for _, b in parts], axis=0)


def coarse_margin(S):
    """How far the twin's S (any shape) stays from MARG_COARSE_S: below S_MARGIN a coarse flag is undecidable between two implementations."""
    return float(np.min(np.abs(np.asarray(S) - COARSE_S)))


# Engine-resident data at 896 items: parity_util.make_problem(model, 70, 896, 3, ...), two tiles and a tail of six; 6 sweeps with 2 burn-in, and one LOO case of 30
# sweeps with 5 burn-in.  On the CPU the oracle's chain of the same inputs stands for the fp64 engine's (they agree to 1e-7 at 896 items: tests/test_gpu_wide_items.py).
ENGINE_N, ENGINE_SWEEPS, ENGINE_BURNIN, LOO_SWEEPS, LOO_BURNIN, ENGINE_SEED = 70, 6, 2, 30, 5, 41
ENGINE_MODELS = ("rtirt", "cross", "latentqr")


@functools.lru_cache(maxsize=None)
def engine_inputs(model):
    Y, logT, X, init, _ = pu.make_problem(model, ENGINE_N, J_MAX, 3, seed=ENGINE_SEED)
    return Y, logT, X, init


def oracle_problem(model, sweeps, burnin):
    """The Problem of an engine case with the oracle's chain in the engine's place: its post-burn-in item-trace rows [a b lambda sig2t | small part of qr]."""
    Y, logT, X, init = engine_inputs(model)
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=Q_RT, cov2one=model not in ("latentqr", "latent"), seed=1234)
    with pu.oracle_threads(16):
        t = op.run(sweeps)
    rows = np.ascontiguousarray(np.hstack([t["ra"][:, ENGINE_N:], t["rt"][:, ENGINE_N:], t["qr"]])[burnin:])
    return Problem(model=model, code=CODE[model], Y=Y, logT=logT, X=X if model == "latentqr" else _kernel_x(model, X), rows=rows, obs=None, Q=WIDE_Q, K=K_DRAWS,
                   seed=PV_SEED)

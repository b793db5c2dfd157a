"""Helpers shared by the tests of the plausible values (tests/test_pv_host.py, tests/test_gpu_plausible_values.py): the figures by which a table of draws is
compared with the scores of the same subjects, and the condition under which two implementations of the Gumbel-max choice must pick the same node."""
import numpy as np

import marginal_util as mu
import parity_util as pu

GAP_MIN = 1e-8          # a draw whose two best keys lie closer than this is undecidable between the kernel and the twin (e_q agrees to about 1e-12)


# The shapes at which tests/test_gpu_plausible_values.py compares pv_kernel with the twin: (model, J, Q, K, rows), every one at N = 70 (two full tiles of 32 subjects
# and a part tile with idle lanes), F = 3 and CASE_SEED.  J = 5 leaves item lanes idle, J = 9 puts two items on one lane; Q = 9 is fewer nodes than one lane chunk,
# Q = 129 two chunks per lane; K = 1, 5 and 3 x rows (rows repeat); rows = 1 and 7.  tests/test_pv_host.py checks on the CPU that the twin has no draw closer than
# GAP_MIN at these seeds.
CASE_N, CASE_F, CASE_SEED, CASE_DATA_SEED = 70, 3, 20191, 81
CASES = [(m, 9, 61, 5, 7) for m in mu.MODELS] + [("rtirt", 5, 9, 1, 7), ("cross", 5, 129, 21, 7), ("mlirt", 9, 129, 1, 1), ("latent", 5, 9, 3, 1), ("null", 9, 9, 21, 7),
                                                  ("rtirt", 9, 129, 5, 1)]


def case_problem(model, J, R):
    return problem(model, CASE_N, J, CASE_F, R, seed=CASE_DATA_SEED)


def pkg():
    return pu.ge.load_package()


def kernel_x(model, X):
    return X if model in ("mlirt", "rtirt", "latent") else None


def problem(model, N, J, F, R, seed):
    """(Y, logT, X as the kernels see it, rows) of marginal_util's random rows and data."""
    rows = mu.make_rows(model, J, F, R, seed=seed)
    Y, logT, X = mu.make_data(model, N, J, F, seed=seed)
    return Y, logT, kernel_x(model, X), rows


def moment_figures(pv, sc, rt):
    """The draws (an OutputPv with theta, zeta (N, K)) against the scores (an OutputScores) of the same subjects and rows.  Returns a dict of the largest, over the
    subjects, of: z_theta, z_zeta = |mean_k draw - score| / (sd / sqrt(K));  var_theta, var_zeta = |sample variance / sd^2 - 1|;
    cov = |sample covariance - cov| / (thetaSd zetaSd).  The zeta figures are left out for a model without zeta."""
    K = pv.theta.shape[1]
    out = dict(z_theta=float(np.max(np.abs(pv.theta.mean(axis=1) - sc.theta) / (sc.thetaSd / np.sqrt(K)))),
               var_theta=float(np.max(np.abs(pv.theta.var(axis=1, ddof=1) / sc.thetaSd ** 2 - 1.0))))
    if rt:
        dt, dz = pv.theta - pv.theta.mean(axis=1, keepdims=True), pv.zeta - pv.zeta.mean(axis=1, keepdims=True)
        out.update(z_zeta=float(np.max(np.abs(pv.zeta.mean(axis=1) - sc.zeta) / (sc.zetaSd / np.sqrt(K)))),
                   var_zeta=float(np.max(np.abs(pv.zeta.var(axis=1, ddof=1) / sc.zetaSd ** 2 - 1.0))),
                   cov=float(np.max(np.abs(np.sum(dt * dz, axis=1) / (K - 1) - sc.cov) / (sc.thetaSd * sc.zetaSd))))
    return out


def row_figures(theta, rk, E, V):
    """theta (N, K) against the moments E, V (N, K) of the row r_k (K,) each draw was made from: the largest, over subjects and rows, of
    z = |mean of the row's draws - E| / sqrt(V / m) and var = |sample variance of the row's draws / V - 1|, m = the draws of the row."""
    z = var = 0.0
    for r in np.unique(rk):
        ks = np.nonzero(rk == r)[0]
        t, e, v = theta[:, ks], E[:, ks[0]], V[:, ks[0]]
        z = max(z, float(np.max(np.abs(t.mean(axis=1) - e) / np.sqrt(v / ks.size))))
        var = max(var, float(np.max(np.abs(t.var(axis=1, ddof=1) / v - 1.0))))
    return dict(z=z, var=var)

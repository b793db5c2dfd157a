"""Helpers shared by the posterior predictive tests (tests/test_predictive_host.py, tests/test_gpu_predictive.py): the thresholds of the 2pl-against-1pl misfit case
(fixed on the CPU with the oracle chain, see test_predictive_host.py's docstring), the law checks and the comparison of two OutputPpc objects."""
import numpy as np

MODELS = ["mlirt", "rtirt", "crossqr", "latentqr", "null", "cross", "latent"]

# waic_util.spread_problem (600 x 12, 200 sweeps, 100 replicates): the item RA ppp_mid values
BAND_2PL = (0.2, 0.8)          # every item under the 2pl fit (observed 0.44 ... 0.61; the Monte Carlo sd of a ppp near 1/2 from 100 replicates is 0.05)
LOW_A_1PL_MAX = 0.1            # the lowest-discrimination item under the 1pl fit (observed 0.00)
HIGH_A_1PL_MIN = 0.9           # the highest-discrimination item under the 1pl fit (observed 1.00)

MARGIN = 1e-9                  # a count is compared exactly when the unit's smallest non-zero |D_rep - D_obs| exceeds this share of the compared magnitudes
MAX_EXCLUDED = 1e-3            # share of a case's units the margin rule may exclude


def check_counts(P):
    """n_gt <= n_ge <= R, whole numbers; the data set's means are the sums of the items' and of the subjects' means."""
    for a in (P.item, P.subj, P.total):
        for c in range(a.shape[0]):
            if np.all(np.isnan(a[c])):
                continue
            assert np.all(a[c, 0] == np.round(a[c, 0])) and np.all(a[c, 1] == np.round(a[c, 1]))
            assert np.all(0 <= a[c, 1]) and np.all(a[c, 1] <= a[c, 0]) and np.all(a[c, 0] <= P.R)
    for c in range(2):
        if np.all(np.isnan(P.total[c])):
            continue
        for q in (2, 3):
            t = P.total[c, q]
            assert abs(P.item[c, q].sum() - t) <= 1e-11 * abs(t) and abs(P.subj[c, q].sum() - t) <= 1e-11 * abs(t), (c, q)


def check_rt_law(P, N, J):
    """D^T_rep of a subject is a chi^2 with nItem degrees of freedom (mean nItem, variance 2 nItem): the mean over subjects and replicates within five standard errors."""
    got, bound = float(P.subj[1, 3].mean()), 5.0 * np.sqrt(2.0 * J / (N * P.R))
    print(f"  RT law: mean D^T_rep {got:.5f} against nItem = {J}, bound {bound:.5f}")
    assert abs(got - J) <= bound


def check_score_law(P, pbar, N):
    """pbar[i, j]: the mean over the replicate rows of p_ij, evaluated by the caller from the traces.  T_rep of an item is a sum of N Bernoulli draws per row (variance
    at most N / 4): its mean over R rows lies within 5 sqrt(N / (4 R)) of sum_i pbar_ij."""
    err, bound = np.abs(P.item[2, 3] - pbar.sum(axis=0)), 5.0 * np.sqrt(N / (4.0 * P.R))
    print(f"  score law: max |mean T_rep - sum_i mean p_ij| {err.max():.4f}, bound {bound:.4f}")
    assert np.all(err <= bound)


def mean_p(ra, N, J, rows):
    """Mean over trace rows `rows` (pairs (iteration, chain)) of p_ij = 1 / (1 + exp(-a_j (theta_i - b_j))) from a Post.ra array (nIter, N + 2 J, nChain)."""
    acc = np.zeros((N, J))
    for it, l in rows:
        r = ra[it, :, l]
        acc += 1.0 / (1.0 + np.exp(-(r[N:N + J][None, :] * (r[:N][:, None] - r[N + J:N + 2 * J][None, :]))))
    return acc / len(rows)


def replicate_rows(nIter, nChain, nBurnin, thin):
    post = [(it, l) for it in range(nBurnin, nIter) for l in range(nChain)]
    return post[::thin]


def excluded_units(host):
    """Units (per unit kind and component) whose counts the margin rule takes out of the exact comparison."""
    return {k: ~(v > MARGIN) for k, v in host.margin.items()}


def assert_equals_twin(dev, host, tol=1e-10, what=""):
    """Means to tol relative; counts exactly for every unit the margin rule keeps, and the rule keeps all but MAX_EXCLUDED of the case's units."""
    assert dev.R == host.R
    ex = excluded_units(host)
    n_units = n_ex = 0
    worst = 0.0
    for name, d, h, e in (("item", dev.item, host.item, ex["item"]), ("subject", dev.subj, host.subj, ex["subject"]), ("total", dev.total, host.total, ex["total"])):
        for c in range(d.shape[0]):
            if np.all(np.isnan(h[c])):
                assert np.all(np.isnan(d[c])), (name, c)
                continue
            keep = ~np.atleast_1d(e[c])
            n_units += keep.size
            n_ex += int((~keep).sum())
            for q in (0, 1):
                assert np.array_equal(np.atleast_1d(d[c, q])[keep], np.atleast_1d(h[c, q])[keep]), (what, name, c, q)
            for q in (2, 3):
                rel = np.max(np.abs(d[c, q] - h[c, q]) / np.maximum(np.abs(h[c, q]), 1e-300))      # (an item nobody solved: T_obs = 0 on both sides)
                worst = max(worst, float(rel))
    print(f"{what}: R {dev.R}, max rel err of the means {worst:.3g}, units excluded by the margin rule {n_ex} of {n_units}")
    assert worst <= tol
    assert n_ex <= MAX_EXCLUDED * n_units

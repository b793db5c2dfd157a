"""Helpers shared by the tests of incomplete response patterns (tests/test_obs_host.py, tests/test_gpu_incomplete.py): the observed-mask patterns the
issue names, the data set and the rows of one subject reduced to its observed items, and the comparison of two results."""
import numpy as np

import marginal_util as mu

PATTERNS = ("all", "none", "last", "from8", "alternating", "random")


def pattern(name, J, g):
    """One subject's mask (J,) uint8: all, none, the last item only, only the items >= 8 (empty below J = 9), alternating (items 0, 2, ...), random halves."""
    o = np.zeros(J, dtype=np.uint8)
    if name == "all":
        o[:] = 1
    elif name == "last":
        o[J - 1] = 1
    elif name == "from8":
        o[8:] = 1
    elif name == "alternating":
        o[::2] = 1
    elif name == "random":
        o[:] = g.uniform(size=J) < 0.5
    elif name != "none":
        raise ValueError(name)
    return o


def masks(N, J, seed):
    """obs (N, J) uint8: subject i has pattern i mod 6 (the random ones differ from subject to subject), so with N = 33 every pattern occurs in both tiles' waves and
    n_i = 0, 1, J - 8, ceil(J / 2), about J / 2 and J stand side by side."""
    g = np.random.default_rng(seed)
    return np.stack([pattern(PATTERNS[i % len(PATTERNS)], J, g) for i in range(N)])


def reduce_rows(model, rows, J, items):
    """The table restricted to the columns of `items` (rising): a, b, lambda, sig2t, and Cross's rho, subset in the same order; the structural part as it is."""
    items = np.asarray(items, dtype=np.int64)
    parts = [rows[:, k * J + items] for k in range(4)]
    tail = rows[:, 4 * J:]
    if model == "cross":
        parts.append(tail[:, items])
        tail = tail[:, J:]
    return np.ascontiguousarray(np.hstack(parts + [tail]))


def reduced_subject(model, Y, logT, X, rows, obs, i):
    """(Y, logT, X, rows) of subject i as a one-subject data set that has only the items O_i; None when n_i = 0 (a data set has at least one item)."""
    items = np.nonzero(obs[i])[0]
    if items.size == 0:
        return None
    J = Y.shape[1]
    return (np.ascontiguousarray(Y[i:i + 1, items]), None if logT is None else np.ascontiguousarray(logT[i:i + 1, items]), None if X is None else X[i:i + 1],
            reduce_rows(model, rows, J, items))


def poison(Y, logT, obs):
    """Copies of Y and logT with the unobserved cells set to 255 and NaN."""
    O = obs != 0
    return np.where(O, Y, 255).astype(np.uint8), None if logT is None else np.where(O, logT, np.nan)


def rel(got, ref):
    """The largest |got - ref| / max(|ref|, 1); NaN must stand against NaN."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1.0))) if np.any(ok) else 0.0


def kernel_x(model, X):
    return X if model in ("mlirt", "rtirt", "latent") else None


def problem(model, N, J, R, seed, F=3):
    """(Y, logT, X as the kernels see it, rows, obs) of marginal_util's random rows and data with masks()."""
    rows = mu.make_rows(model, J, F, R, seed=seed)
    Y, logT, X = mu.make_data(model, N, J, F, seed=seed)
    return Y, logT, kernel_x(model, X), rows, masks(N, J, seed + 7)


# The shapes at which tests/test_gpu_incomplete.py compares the MASKED pv_kernel with the twin: (J, R, Q, K) for every model at N = 33 and PV_SEED, obs = masks().
# tests/test_obs_host.py checks on the CPU that the twin has no draw closer than pv_util.GAP_MIN at these seeds.
PV_N, PV_SEED, PV_DATA_SEED = 33, 20191, 91
PV_CASES = [(1, 3, 61, 5), (9, 3, 61, 5), (65, 3, 61, 5), (9, 1, 3, 3)]


def pv_problem(model, J, R):
    return problem(model, PV_N, J, R, seed=PV_DATA_SEED)

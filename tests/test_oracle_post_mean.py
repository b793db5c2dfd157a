"""The helpers the Post.mean tests stand on (parity_util.decode_rows / expected_mean / mean_excess), checked without a GPU: the column
mapping against the oracle's own state arrays, the mean against closed forms."""
import math

import numpy as np
import pytest

import parity_util as pu

N, J, F = 23, 5, 3
ARR = dict(theta="theta", a="a", b="b", zeta="zeta", lambda_="lambda_", sig2t="sig2t", beta="beta", sigp="Sigp", rho="rho", nu="nu")
FIELDS = {"mlirt": {"theta", "a", "b", "beta"},
          "rtirt": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"},
          "null": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"},
          "cross": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "rho", "sigp"},
          "crossqr": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "rho", "sigp", "nu"},
          "latent": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp"},
          "latentqr": {"theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp", "nu"}}


@pytest.mark.parametrize("model", list(pu.MODELS))
def test_decode_rows_is_the_oracle_state_of_the_last_row(model):
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F, seed=5)
    op = pu.OracleProblem(model, Y, logT, X, init, qRt=0.85, cov2one=model not in ("latentqr", "latent"))
    tr = op.run(4, with_nu=model in pu.NU_MODELS)
    f = pu.decode_rows(model, N, J, F, tr["ra"], None if model == "mlirt" else tr["rt"], tr["qr"])
    assert set(f) == FIELDS[model]
    sizes = dict(theta=N, a=J, b=J, zeta=N, lambda_=J, sig2t=J, sigp=4, rho=J, nu={"crossqr": N * J, "latentqr": N}.get(model),
                 beta={"mlirt": F + 1, "rtirt": 2 * (F + 1), "null": 2 * (F + 1), "latent": F + 2, "latentqr": F + 2}.get(model))
    for k, v in f.items():
        assert v.shape == (4, sizes[k]), k
        assert np.array_equal(v[-1], op.arr[ARR[k]]), (model, k)          # bit for bit
        assert k == "sigp" or (k == "beta" and model == "null") or len(np.unique(v)) > 4, (model, k)      # a live block, not a constant
    if model == "null":
        assert np.all(f["beta"] == 0)
    if model == "crossqr":           # vec(nu) is column-major N x J: cell (i, j) at i + N j
        nu = f["nu"][-1].reshape(N, J, order="F")
        assert nu[3, 2] == op.arr["nu"][3 + N * 2]
    if model in pu.NU_MODELS:        # without the nu block the same rows decode without nu
        g = pu.decode_rows(model, N, J, F, tr["ra"], tr["rt"], tr["qr"][:, :tr["qr"].shape[1] - f["nu"].shape[1]])
        assert set(g) == FIELDS[model] - {"nu"} and np.array_equal(g["sigp"], f["sigp"])
    with pytest.raises(ValueError):
        pu.decode_rows(model, N, J, F, tr["ra"], tr["rt"], tr["qr"][:, :-1])
    with pytest.raises(ValueError):
        pu.decode_rows(model, N + 1, J, F, tr["ra"], tr["rt"], tr["qr"])


def test_trace_rows_orders_the_chains_round_robin():
    tr = np.zeros((4, 2, 3), order="F")                    # (nIter, width, nChain)
    for m in range(4):
        for l in range(3):
            tr[m, :, l] = (m * 3 + l, -(m * 3 + l))
    rows = pu.trace_rows(tr)
    assert rows.shape == (12, 2) and np.array_equal(rows[:, 0], np.arange(12)) and np.array_equal(rows[:, 1], -np.arange(12))
    assert pu.trace_rows(rows) is rows


@pytest.mark.parametrize("n_chain", [1, 3])
def test_expected_mean_closed_forms(n_chain):
    c = np.array([0.1, -1e300, 3.0e-310, 0.0])           # a constant trace: the mean is the constant, exactly
    for n_iter, nb in ((7, 0), (7, 3), (7, 6)):
        mean, asum, n = pu.expected_mean(dict(x=np.tile(c, (n_iter * n_chain, 1))), nb, n_chain)
        assert n == (n_iter - nb) * n_chain
        assert np.array_equal(mean["x"], c.astype(np.longdouble))
        assert np.array_equal(asum["x"], np.abs(c).astype(np.longdouble) * n)
        assert np.all(pu.mean_excess(c, mean["x"], asum["x"], n) == 0)
    # two iterations: row r holds base + 3 r, so every block of n_chain rows has a dyadic mean
    base = np.array([0.375, -1024.5])
    rows = np.stack([base + 3.0 * r for r in range(2 * n_chain)])
    mean, asum, n = pu.expected_mean(dict(x=rows), 0, n_chain)
    assert n == 2 * n_chain and np.array_equal(mean["x"], (base + 1.5 * (2 * n_chain - 1)).astype(np.longdouble))
    mean, asum, n = pu.expected_mean(dict(x=rows), 1, n_chain)
    assert n == n_chain and np.array_equal(mean["x"], (base + 3.0 * n_chain + 1.5 * (n_chain - 1)).astype(np.longdouble))
    assert np.array_equal(asum["x"], np.abs(rows[n_chain:]).sum(axis=0).astype(np.longdouble))
    with pytest.raises(ValueError):
        pu.expected_mean(dict(x=rows), 2, n_chain)


def test_expected_mean_carries_no_fp64_summation_error_and_the_bound_sees_one_row():
    g = np.random.default_rng(3)
    x = g.standard_normal((40, 50)) * np.exp(g.uniform(-20, 20, (1, 50)))
    mean, asum, n = pu.expected_mean(dict(x=x), 8, 1)
    exact = np.array([math.fsum(x[8:, k]) for k in range(50)])         # the correctly rounded sums
    assert np.all(np.abs(mean["x"] * n - exact) <= np.abs(exact) * 2.0 ** -52)
    assert np.all(np.abs((mean["x"] * n).astype(np.float64) - exact) <= np.spacing(np.abs(exact)))
    naive = x[8:].sum(axis=0) * (1.0 / n)                               # fp64 in any order: inside the bound
    assert pu.mean_excess(naive, mean["x"], asum["x"], n).max() <= 1.0
    for wrong in (x[7:].sum(axis=0) / (n + 1), x[9:].sum(axis=0) / (n - 1), x[7:-1].sum(axis=0) / n):        # one row off at either end
        assert pu.mean_excess(wrong, mean["x"], asum["x"], n).min() > 1e6
    z = pu.mean_excess(np.array([0.0, 1e-300]), np.zeros(2, np.longdouble), np.zeros(2, np.longdouble), 5)
    assert z[0] == 0 and np.isinf(z[1])

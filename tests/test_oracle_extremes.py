"""The adversarial problems of tests/test_gpu_data_extremes.py, checked without a GPU: each generator reaches the region it is named for
(pg_cell_coverage on its initial state and on the oracle's state after the sweeps the GPU tests compare), and the oracle's chains on them
stay finite.  A generator change that stopped reaching its region fails here, not silently in the GPU suite."""
import numpy as np
import pytest

import parity_util as pu

N, J = 1200, 24          # the size the GPU tests use (a persistent launch; 28 800 cells)
T = 8

CASES = [(k, m) for k in pu.EXTREME_KINDS for m in pu.extreme_models(k)]


def _oracle(kind, model):
    Y, logT, X, init, _ = pu.make_extreme_problem(kind, model, N, J)
    op = pu.OracleProblem(model, Y, logT, X, init, cov2one=model not in ("latentqr", "latent"))
    return Y, logT, X, init, op


def test_every_model_has_every_kind_it_can_take():
    assert pu.extreme_models("separated") == list(pu.MODELS) and pu.extreme_models("degenerate") == list(pu.MODELS)
    assert "mlirt" not in pu.extreme_models("rt_offset") and len(pu.extreme_models("rt_offset")) == 6
    assert sorted(pu.extreme_models("x_offset")) == sorted(["mlirt", "rtirt", "latentqr", "latent"])
    with pytest.raises(ValueError):
        pu.make_extreme_problem("x_offset", "cross", N, J)


def test_pg_cell_coverage_bins():
    c = pu.pg_cell_coverage(np.array([0.0, 1.0 / 8.0 - 1e-12, 1.0 / 8.0, 16.0 - 1e-9, 16.0, 96.0, 1500.0]), np.array([1.0]), np.array([0.0]))
    assert c["hist"][0] == 2 and c["hist"][1] == 1 and c["hist"][127] == 1 and c["hist"].sum() == 4
    assert c["bins_hit"] == 3 and c["frac_ge8"] == pytest.approx(3 / 7) and c["n_ge48"] == 2 and c["n_gt745"] == 1 and c["zmax"] == 750.0


@pytest.mark.parametrize("model", pu.extreme_models("separated"))
def test_separated_reaches_the_reference_form_and_every_bin(model):
    _, _, _, init, op = _oracle("separated", model)
    for st in (init, None):
        if st is None:
            op.run(T)
            st = op.arr
        c = pu.pg_cell_coverage(st["theta"], st["a"], st["b"])
        assert c["frac_ge8"] >= 0.02, c["frac_ge8"]
        assert c["bins_hit"] == 128, np.flatnonzero(c["hist"] == 0)


@pytest.mark.parametrize("model", pu.extreme_models("saturated"))
def test_saturated_reaches_underflow_and_the_nan_ratio(model):
    _, _, _, init, op = _oracle("saturated", model)
    c = pu.pg_cell_coverage(init["theta"], init["a"], init["b"])
    assert c["n_ge48"] > 0 and c["n_gt745"] > 0 and c["eta_max"] > 1400.0
    assert c["frac_ge8"] >= 0.02 and c["bins_hit"] == 128
    r = op.run(1)
    c = pu.pg_cell_coverage(op.arr["theta"], op.arr["a"], op.arr["b"])     # the state the sweep kernel's own omega draw and log-likelihood see
    assert c["n_ge48"] > 0 and c["n_gt745"] > 0 and c["eta_max"] > 1400.0, c
    r2 = op.run(1)
    assert all(np.isfinite(v).all() for v in list(r.values()) + list(r2.values()))
    assert np.isfinite(op.loglik())


def test_degenerate_patterns():
    Y, _, _, _, _ = pu.make_extreme_problem("degenerate", "rtirt", N, J)
    assert np.all(Y[:, 0:2] == 1) and np.all(Y[:, 2:4] == 0) and Y[:, 4].sum() == 1
    assert np.all(Y[0:3, 0:2] == 1) and np.all(Y[0:3, 5:] == 1)         # all-correct subjects (the items are exact: not on the all-0 items)
    assert np.all(Y[3:6, 2:] == 0)


@pytest.mark.parametrize("model", pu.extreme_models("rt_offset"))
def test_rt_offset_item_keeps_its_tiny_residual_variance(model):
    """Item 0's within-item residual variance ~1e-4 (where the expanded-square RT statistics cancel by 1e4) must be where the compared chain
    is, not only in the data: the oracle's sigma2_t[0] over the sweeps the GPU tests compare.  (CrossQr: sigma2_t is the scale of an
    asymmetric Laplace residual -- of the order of the mean absolute residual, 1e-2 here -- not a variance.)"""
    _, _, _, init, op = _oracle("rt_offset", model)
    r = op.run(T)
    s0 = r["rt"][:, N + J]
    bound = 5e-3 if model == "crossqr" else 1e-3
    assert np.all(s0 <= bound), s0
    assert np.all(r["rt"][:, N + J + 2:] > 10 * bound)        # the other items stay ordinary


def test_rt_offset_data():
    for model in pu.extreme_models("rt_offset"):
        _, logT, _, init, tp = pu.make_extreme_problem("rt_offset", model, N, J)
        assert 7.0 < logT.mean() < 9.0
        assert np.ptp(logT[:, 1]) == 0.0
        assert np.max(np.abs(init["zeta"] - (tp.zeta + 3.0))) < 1e-2            # zeta offset by +3, absorbed into lambda
        assert 10.0 < init["lam"].mean() < 12.0 and init["sig2t"][0] == 1e-4


def test_x_offset_data():
    for model in pu.extreme_models("x_offset"):
        _, _, X, _, _ = pu.make_extreme_problem("x_offset", model, N, J)
        assert X.min(axis=0)[0] >= 20.0 and X.max(axis=0)[0] <= 70.0
        assert set(np.unique(X[:, 1])) <= {0.0, 1.0} and 0.02 < X[:, 1].mean() < 0.08


@pytest.mark.parametrize("kind,model", CASES)
def test_oracle_chains_stay_finite(kind, model):
    """The chains the GPU tests compare against: the free-running oracle over the sweeps they use, every trace and the state finite."""
    _, _, _, _, op = _oracle(kind, model)
    r = op.run(T, with_nu=model in ("latentqr", "crossqr"))
    for k, v in r.items():
        assert np.isfinite(v).all(), k
    for k, v in op.arr.items():
        assert np.isfinite(v).all(), k

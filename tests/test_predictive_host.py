"""Posterior predictive checks on the host (no GPU): getPpcHost, the numpy twin the device path is tested against.  Its Philox4x32-10 and its uniform / normal
variates against the oracle library's; its counts and sums on an oracle chain of every model; the laws of the replicates, checked without the twin's draw code
(the chi^2 mean of D^T_rep, the item scores against the Bernoulli means); no unit decided within rounding at the shapes of tests/test_gpu_predictive.py;
calibration and power on the 2pl-against-1pl data of waic_util.spread_problem; argument checks of the public interface.

Values observed with the oracle chain (600 x 12, 200 sweeps, burn-in 100, R = 100 replicates, seed 1234), from which ppc_util's thresholds were chosen:
  2pl fit: item RA ppp_mid 0.49 0.50 0.51 0.44 0.61 0.58 0.51 0.49 0.57 0.50 0.54 0.60 (all within 0.44 ... 0.61; band asserted: 0.2 ... 0.8), total 0.54
  1pl fit: item RA ppp_mid 0.00 0.00 0.03 0.62 0.51 1.00 1.00 0.99 0.98 1.00 1.00 1.00 -- the lowest-discrimination item 0.00 (asserted <= 0.1), the highest 1.00
           (asserted >= 0.9), total 0.96; the item scores stay central under both fits (0.36 ... 0.68): the score is no test of the slopes."""
import ctypes as C
import types

import numpy as np
import pytest

import parity_util as pu
import ppc_util as ppu
import waic_util as wu

pkg = pu.ge.load_package()
G = pkg.twins


def test_numpy_philox_equals_the_oracle_block():
    o, g = pu.oracle(), np.random.default_rng(3)
    ctr = g.integers(0, 2 ** 32, (200, 4), dtype=np.uint64).astype(np.uint32)
    key = g.integers(0, 2 ** 32, (200, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    out = np.zeros(4, dtype=np.uint32)
    w = G._philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 0, 0)      # (vectorised over the counters; the key is one per call)
    for n in range(len(ctr)):
        o.orc_philox(ctr[n].ctypes.data_as(C.c_void_p), key[n].ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        got = G._philox4x32_10(ctr[n, 0], ctr[n, 1], ctr[n, 2], ctr[n, 3], key[n, 0], key[n, 1])
        assert [int(v) for v in got] == [int(v) for v in out], n
    o.orc_philox(ctr[5].ctypes.data_as(C.c_void_p), np.zeros(2, dtype=np.uint32).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert [int(v[5]) for v in w] == [int(v) for v in out]


@pytest.mark.parametrize("seed,sweep", [(1234, 1), (0xFEDCBA9876543210, 4_000_000_000)])
def test_twin_uniform_and_normal_equal_the_oracle_variates_at_site_14(seed, sweep):
    n = 5000
    u, z = pu.orc_sample(0, n, seed=seed, site=14, sweep=sweep), pu.orc_sample(1, n, seed=seed, site=14, sweep=sweep)
    w = G._philox4x32_10(np.arange(n), 0, sweep, G._ppc_stream_word3(0), seed, seed >> 32)
    assert G._ppc_stream_word3(0) == 14 << 24 and G._ppc_stream_word3(3) == (14 << 24) | (3 << 16)
    assert np.max(np.abs(G._ppc_uniform(w[0]) - u)) <= 1e-15
    assert np.max(np.abs(G._ppc_normal(w[0], w[1]) - z)) <= 1e-15        # the oracle's normal takes the stream's first two words


@pytest.mark.parametrize("model", ppu.MODELS)
def test_twin_on_an_oracle_chain_counts_sums_and_laws(model):
    N, J, T, burn = 400, 9, 24, 8
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=9)
    M = wu.oracle_sampler(model, Y, logT, X, init, T, nBurnin=burn)
    for thin in (1, 3):
        P = pkg.getPpcHost(M, thin=thin, seed=1234)
        assert P.R == len(ppu.replicate_rows(T, 1, burn, thin)) and P.item.shape == (3, 4, J) and P.subj.shape == (2, 4, N) and P.total.shape == (2, 4)
        ppu.check_counts(P)
        assert np.array_equal(P.item[2, 2], Y.sum(axis=0))
        if model == "mlirt":
            assert np.all(np.isnan(P.item[1])) and np.all(np.isnan(P.subj[1])) and np.all(np.isnan(P.total[1]))
        else:
            ppu.check_rt_law(P, N, J)
        ppu.check_score_law(P, ppu.mean_p(M.Post.ra, N, J, ppu.replicate_rows(T, 1, burn, thin)), N)
        assert np.all(P.ppp_mid("subject", "ra") <= P.ppp("subject", "ra")) and 0.0 < P.ppp("total", "ra") <= 1.0
    # other seeds and sweep origins give other replicates; the same give the same
    a, b, c = pkg.getPpcHost(M, seed=1234), pkg.getPpcHost(M, seed=1235), pkg.getPpcHost(M, seed=1234, sweep0=2)
    assert np.array_equal(a.subj, pkg.getPpcHost(M, seed=1234).subj, equal_nan=True)
    assert not np.array_equal(a.subj[0], b.subj[0]) and not np.array_equal(a.subj[0], c.subj[0])


@pytest.mark.parametrize("model", ppu.MODELS)
@pytest.mark.parametrize("shape", [(1001, 17), (4000, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_unit_is_decided_within_rounding_at_the_gpu_test_shapes(model, shape):
    """tests/test_gpu_predictive.py compares counts exactly except for units whose smallest non-zero |D_rep - D_obs| is within 1e-9 of the compared magnitudes: on the
    oracle chain at those shapes, seeds and thinnings (18 sweeps, 9 post-burn-in) there is no such unit."""
    N, J = shape
    Y, logT, X, init, tp = pu.make_problem(model, N, J, 3, seed=17)
    M = wu.oracle_sampler(model, Y, logT, X, init, 18, nBurnin=9)
    for thin in (1, 2):
        P = pkg.getPpcHost(M, thin=thin, seed=1234)
        ex = ppu.excluded_units(P)
        worst = min(float(np.min(v)) for v in P.margin.values())
        print(f"{model} {N}x{J} thin {thin}: smallest margin {worst:.3g}")
        assert not any(np.any(v) for v in ex.values())


def test_calibration_and_power_on_spread_discriminations():
    Y, X, init = wu.spread_problem()
    fit = {onepl: pkg.getPpcHost(wu.oracle_sampler("mlirt", Y, None, X, init, wu.SPREAD_ITER, onepl=onepl), seed=1234) for onepl in (False, True)}
    for onepl, P in fit.items():
        print(("1pl" if onepl else "2pl"), "item RA ppp_mid", np.round(P.ppp_mid("item", "ra"), 3), "total", P.ppp_mid("total", "ra"))
    mid = fit[False].ppp_mid("item", "ra")
    assert np.all(mid > ppu.BAND_2PL[0]) and np.all(mid < ppu.BAND_2PL[1])
    mid = fit[True].ppp_mid("item", "ra")               # items in order of their true discrimination 0.25 ... 3
    assert mid[0] <= ppu.LOW_A_1PL_MAX and mid[-1] >= ppu.HIGH_A_1PL_MIN


def test_outputppc_arithmetic():
    P = pkg.OutputPpc(R=4, thin=1, item=np.zeros((3, 4, 2)), subj=np.zeros((2, 4, 3)), total=np.array([[3.0, 1.0, 7.0, 8.0], [4.0, 4.0, 1.0, 2.0]]))
    assert P.ppp("total", "ra") == 0.75 and P.ppp_mid("total", "ra") == 0.5 and P.ppp_mid("total", "rt") == 1.0
    assert P.mean_obs("total", "ra") == 7.0 and P.mean_rep("total", "rt") == 2.0 and P.ppp("item", "score").shape == (2,)
    with pytest.raises(ValueError, match="items only"):
        P.ppp("subject", "score")


def test_public_interface_checks_its_arguments_before_touching_a_device():
    Cond = pkg.setCond(nSubj=10, nItem=3, nFeat=1, nIter=4, nChain=1)
    M = pkg.GibbsMlIrt(Cond)
    for bad in (0, -2, 1.5, "yes"):
        with pytest.raises(ValueError, match="ppc must be"):
            pkg.sample_b(M, ppc=bad)
    with pytest.raises(ValueError, match="chain farm"):
        pkg.sample_b(M, ppc=True, devices=[0])
    with pytest.raises(ValueError, match="chain farm"):
        pkg.sample_b(M, ppc=3, devices=[0])
    with pytest.raises(ValueError, match="run sample"):
        pkg.getPpc(M)
    M.farm = types.SimpleNamespace(close=lambda: None)
    with pytest.raises(ValueError, match="devices="):
        pkg.getPpc(M)
    M.farm = None
    with pytest.raises(ValueError, match="full Post traces"):
        pkg.getPpcHost(types.SimpleNamespace(Cond=Cond, Data=None, Post=types.SimpleNamespace(ra=np.zeros(0)), _model=0, seed=1))
    L = pkg._lib
    for name in ("erm_set_predictive", "erm_predictive_reps", "erm_get_predictive"):
        assert name in L.EXPORTS and hasattr(L.load(), name)

"""Incomplete response patterns on the device (erm_marginal_loglik_masked / erm_score_masked / erm_plausible_values_masked).
Shapes: N in {1, 33} (33: two tiles, one nearly empty), J in {1, 9, 65}, rows in {1, 3}, Q in {3, 61}; subject i has pattern i mod 6 of obs_util.PATTERNS (all, none,
last item only, only items >= 8, alternating, random), so a wave holds subjects with n_i = 0, 1, J - 8, about J / 2 and J side by side; the single subject of N = 1
is the batch's subject 4 (alternating).  All five models.
  1. the MASKED kernels against the masked twins (themselves pinned on the CPU, tests/test_obs_host.py) to 1e-10 relative to max(|ref|, 1), the tolerance of
     tests/test_gpu_scores.py: l, every score column under both weightings; COARSE, row_ess under equal weights, out4 and n_obs exactly.
  2. plausible values: the kernel equals the twin with equal nodes at obs_util.PV_CASES, whose draws are all decidable (pv_util.GAP_MIN; checked on the CPU).
  3. obs = NULL and obs all ones: bit for bit the unmasked entries, for all three products.
  4. a pattern subject against the same subject in a data set that has only its observed items, through the unmasked entry: bit for bit.
  5. poisoned unobserved cells (logT = NaN, Y = 255): bit for bit the clean call; the same poison at an observed cell is refused with the right code.
  6. independence: a subject's result is bit-identical alone, at another position of a batch of 33 (plausible values: at the same index among other subjects),
     when another subject's mask changes, and under ERM_PV_CHUNK = 5.
  7. erm_psis_loo on the masked l (J = 9, 30 rows, N = 33) against psisLooHost on the twin's l within the bound of tests/test_gpu_psis_loo.py.
  8. refusals: the quantile models, an obs value of 2, the NULL and argument cases.
  9. end to end: GibbsRtIrt fitted on a complete 96 x 12 data set on the device, the same respondents scored with a random half of their cells masked."""
import numpy as np
import pytest

import marginal_util as mu
import obs_util as ou
import parity_util as pu
import psis_util as ps
import pv_util as pvu
import score_util as su
from item_pass_util import _engine, _pkg

pytestmark = pytest.mark.gpu

TOL = 1e-10
WEIGHTINGS = ("equal", "likelihood")
SCORE_KEYS = su.COLS + ("coarse",)
PV_KEYS = ("theta", "zeta", "node", "coarse")
ALONE = 4          # the batch's subject that is also scored alone (alternating)


def _same(a, b, keys):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _at(r, i, keys):
    return {k: np.asarray(r[k])[i:i + 1] for k in keys}


def _code(e):
    return int(str(e.value).split()[2].rstrip(":"))


# ------------------------------------------------------------------------------------------------------------ 1. the kernels against the twins
@pytest.mark.parametrize("Q", [3, 61])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("J", [1, 9, 65])
@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_kernels_equal_twin(model, J, R, Q):
    pkg = _pkg()
    L, code = pkg._lib, mu.CODE[model]
    Y, logT, X, rows, obs = ou.problem(model, 33, J, R, seed=100 + J)
    n = obs.sum(axis=1)
    assert {0, 1, J} <= set(n)
    one = slice(ALONE, ALONE + 1)
    sl = lambda a, s: None if a is None else a[s]
    for N, s in ((33, slice(None)), (1, one)):
        m = L.marginal_loglik(code, Y[s], sl(logT, s), sl(X, s), rows, nodes=Q, want_waic=R >= 2, obs=obs[s])
        host_l, host_S = pkg.marginalLogLikHost(code, Y[s], sl(logT, s), sl(X, s), rows, Q, with_S=True, obs=obs[s])
        err = {"l": ou.rel(m["l"], host_l.T)}
        assert np.array_equal(m["nObs"], n[s]) and m["nObs"].dtype == np.int32
        if R >= 2:
            w = pkg.twins.waicFromLogLik(host_l)
            err.update(lppd=ou.rel(m["lppd"], w.lppd_u), p=ou.rel(m["p"], w.p_u), elpd=ou.rel([m["totals"]["elpd"]], [w.elpd]))
            assert (m["totals"]["nUnits"], m["totals"]["nRows"], m["totals"]["nNodes"]) == (N, R, Q)
            assert m["totals"]["nCoarse"] == int(np.sum(np.any(host_S < 2.0, axis=0)))
        for weighting in WEIGHTINGS:
            dev = L.score(code, Y[s], sl(logT, s), sl(X, s), rows, nodes=Q, weighting=weighting, obs=obs[s])
            host = pkg.scoresHost(code, Y[s], sl(logT, s), sl(X, s), rows, Q, weighting, obs=obs[s])
            for c in su.COLS:
                err[f"{weighting[0]}.{c}"] = ou.rel(dev[c], getattr(host, c))
            assert np.array_equal(dev["coarse"], host.coarse) and dev["nCoarse"] == host.nCoarse == int(np.sum(dev["coarse"]))
            assert (dev["nSubj"], dev["nRows"], dev["nNodes"]) == (N, R, Q) and np.array_equal(dev["nObs"], n[s])
            if weighting == "equal":
                assert np.all(dev["rowEss"] == R)
        print(f"{model} N={N} J={J} R={R} Q={Q}: worst {max(err.values()):.3g} ({max(err, key=err.get)})")
        assert all(e <= TOL for e in err.values()), err


# ------------------------------------------------------------------------------------------------------------ 2. plausible values
@pytest.mark.parametrize("J,R,Q,K", ou.PV_CASES)
@pytest.mark.parametrize("model", mu.MODELS)
def test_masked_plausible_values_equal_twin(model, J, R, Q, K):
    pkg = _pkg()
    Y, logT, X, rows, obs = ou.pv_problem(model, J, R)
    host, gap = pkg.plausibleValuesHost(mu.CODE[model], Y, logT, X, rows, K, ou.PV_SEED, Q, with_gap=True, obs=obs)
    assert gap.min() >= pvu.GAP_MIN                                                       # the condition on the inputs: every draw is decidable
    dev = pkg._lib.plausible_values(mu.CODE[model], Y, logT, X, rows, K=K, seed=ou.PV_SEED, nodes=Q, obs=obs)
    assert np.array_equal(dev["node"], host.node) and np.array_equal(dev["coarse"], host.coarse) and np.array_equal(dev["nObs"], obs.sum(axis=1))
    err = dict(theta=ou.rel(dev["theta"], host.theta), zeta=ou.rel(dev["zeta"], host.zeta))
    print(f"{model} J={J} R={R} Q={Q} K={K}: theta {err['theta']:.3g}, zeta {err['zeta']:.3g}; smallest gap {gap.min():.3g}, coarse {dev['nCoarse']}")
    assert all(e <= TOL for e in err.values()) and np.all(np.isfinite(dev["theta"]))
    assert (dev["nSubj"], dev["nRows"], dev["nNodes"], dev["nCoarse"], dev["seed"]) == (ou.PV_N, R, Q, host.nCoarse, ou.PV_SEED)
    wrapped = pkg.drawPlausibleValues(mu.CODE[model], Y, logT, X, rows, K, ou.PV_SEED, Q, obs=obs)
    assert np.array_equal(wrapped.theta, dev["theta"]) and np.array_equal(wrapped.node, dev["node"]) and np.array_equal(wrapped.nObs, dev["nObs"])


# ------------------------------------------------------------------------------------------------------------ 3. NULL and all ones
def _products(L, code, Y, logT, X, rows, Q=61, obs=None, K=5, seed=11):
    """The three products as one dict of arrays: l, the score columns under both weightings, the draws."""
    out = {"l": L.marginal_loglik(code, Y, logT, X, rows, nodes=Q, want_waic=False, obs=obs)["l"]}
    for w in WEIGHTINGS:
        sc = L.score(code, Y, logT, X, rows, nodes=Q, weighting=w, obs=obs)
        out.update({f"{w}.{c}": sc[c] for c in SCORE_KEYS})
    pv = L.plausible_values(code, Y, logT, X, rows, K=K, seed=seed, nodes=Q, obs=obs)
    out.update({f"pv.{c}": pv[c] for c in PV_KEYS})
    return out


@pytest.mark.parametrize("J", [1, 9, 65])
@pytest.mark.parametrize("model", mu.MODELS)
def test_all_cells_observed_is_the_unmasked_entry_bit_for_bit(model, J):
    L = _pkg()._lib
    Y, logT, X, rows, _ = ou.problem(model, 33, J, 3, seed=200 + J)
    ref = _products(L, mu.CODE[model], Y, logT, X, rows)
    got = _products(L, mu.CODE[model], Y, logT, X, rows, obs=np.ones_like(Y))
    assert _same(got, ref, ref.keys()), [k for k in ref if not np.array_equal(got[k], ref[k], equal_nan=True)]


def test_obs_null_is_the_unmasked_entry_bit_for_bit():
    """Each masked entry given obs = NULL through ctypes against its complete sibling called the same way: every output, every bit, and n_obs = n_item."""
    L = _pkg()._lib
    lib = L.load()
    N, J, F, R, Q, K = 33, 9, 3, 3, 61, 5
    Y, logT, X, rows, _ = ou.problem("rtirt", N, J, R, seed=301)
    ref = _products(L, 1, Y, logT, X, rows, K=K, seed=11)
    Yf, lf, Xf = np.asfortranarray(Y), np.asfortranarray(logT), np.asfortranarray(X)
    data = (0, 1, N, J, F, Yf.ctypes.data, lf.ctypes.data, Xf.ctypes.data)
    plain, head = (*data, rows.ctypes.data, R), (*data, None, rows.ctypes.data, R)
    ptrs = lambda bufs: [a.ctypes.data for a in bufs]
    same = lambda got, want: all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    n_obs = np.zeros(N, dtype=np.int32)
    # l with the WAIC outputs (3 rows allow them): l, out10, lppd_u, p_u
    want, got = ([np.zeros((N, R), order="F"), np.zeros(10), np.zeros(N), np.zeros(N)] for _ in range(2))
    assert lib.erm_marginal_loglik(*plain, Q, *ptrs(want)) == 0
    assert lib.erm_marginal_loglik_masked(*head, Q, *ptrs(got), n_obs.ctypes.data) == 0
    assert same(got, want) and np.array_equal(got[0], ref["l"]) and list(want[1][5:7]) == [N, R] and np.all(n_obs == J)
    l = np.empty((N, R), order="F")
    assert lib.erm_marginal_loglik_masked(*head, Q, l.ctypes.data, None, None, None, None) == 0 and np.array_equal(l, ref["l"])      # l alone, n_obs may be NULL
    # the scores under both weightings: score, out4
    for w, name in enumerate(WEIGHTINGS):
        want, got = ([np.zeros((7, N)), np.zeros(4)] for _ in range(2))
        n_obs[:] = 0
        assert lib.erm_score(*plain, Q, w, *ptrs(want)) == 0
        assert lib.erm_score_masked(*head, Q, w, *ptrs(got), n_obs.ctypes.data) == 0
        assert same(got, want) and np.all(n_obs == J) and list(got[1][:3]) == [N, R, Q]
        sc = got[0]
        assert all(np.array_equal(sc[k], np.asarray(ref[f"{name}.{c}"], dtype=np.float64), equal_nan=True) for k, c in enumerate(SCORE_KEYS))
        got = [np.zeros((7, N)), np.zeros(4)]
        assert lib.erm_score_masked(*head, Q, w, *ptrs(got), None) == 0 and same(got, want)                 # n_obs may be NULL
    # the plausible values: pv, node, coarse, out4
    want, got = ([np.zeros((2, K, N)), np.zeros((K, N), dtype=np.int32), np.full(N, -1, dtype=np.int32), np.zeros(4)] for _ in range(2))
    n_obs[:] = 0
    assert lib.erm_plausible_values(*plain, Q, K, 11, *ptrs(want)) == 0
    assert lib.erm_plausible_values_masked(*head, Q, K, 11, *ptrs(got), n_obs.ctypes.data) == 0
    assert same(got, want) and np.all(n_obs == J) and list(got[3][:3]) == [N, R, Q] and set(got[2].tolist()) <= {0, 1}
    pv, node = got[0], got[1]
    assert np.array_equal(pv[0].T, ref["pv.theta"]) and np.array_equal(pv[1].T, ref["pv.zeta"]) and np.array_equal(node.T, ref["pv.node"])


# ------------------------------------------------------------------------------------------------------------ 4. the reduced data set
@pytest.mark.parametrize("J", [9, 65])
@pytest.mark.parametrize("model", mu.MODELS)
def test_pattern_subject_equals_the_reduced_subject_bit_for_bit(model, J):
    """The order of every floating-point operation is the same in the two instantiations, so every bit is expected; the worst relative difference is printed
    before it is asserted to be 0."""
    L, code = _pkg()._lib, mu.CODE[model]
    N, R, K = 12, 3, 5
    Y, logT, X, rows, obs = ou.problem(model, N, J, R, seed=400 + J)
    got = _products(L, code, Y, logT, X, rows, obs=obs, K=K)
    worst, differing = 0.0, []
    for i in range(N):
        red = ou.reduced_subject(model, Y, logT, X, rows, obs, i)
        if red is None:
            continue
        Yr, lr, Xr, rr = red
        tile = lambda a: None if a is None else np.repeat(a, i + 1, axis=0)                # the subject at index i of the reduced data set as well: the draws' counter
        ref = _products(L, code, tile(Yr), tile(lr), tile(Xr), rr, K=K)
        for k in ref:
            g, r = np.asarray(got[k])[i], np.asarray(ref[k])[i]
            if not np.array_equal(g, r, equal_nan=True):
                differing.append((i, k))
            if np.asarray(g).dtype.kind == "f":
                worst = max(worst, ou.rel(g, r))
    print(f"{model} J={J}: worst relative difference from the reduced subject {worst:.3g}; differing {differing[:8]}")
    assert not differing and worst == 0.0


# ------------------------------------------------------------------------------------------------------------ 5. poison
@pytest.mark.parametrize("model", ["mlirt", "rtirt", "cross"])
def test_unobserved_cells_are_never_read(model):
    L, code = _pkg()._lib, mu.CODE[model]
    Y, logT, X, rows, obs = ou.problem(model, 33, 9, 3, seed=500)
    Yp, lp = ou.poison(Y, logT, obs)
    clean, dirty = _products(L, code, Y, logT, X, rows, obs=obs), _products(L, code, Yp, lp, X, rows, obs=obs)
    assert _same(dirty, clean, clean.keys())
    i, j = 0, 5                                                                            # subject 0 observes every cell
    calls = (lambda y, t: L.marginal_loglik(code, y, t, X, rows, obs=obs), lambda y, t: L.score(code, y, t, X, rows, obs=obs),
             lambda y, t: L.plausible_values(code, y, t, X, rows, obs=obs))
    for call in calls:
        yb = Yp.copy(); yb[i, j] = 255
        with pytest.raises(L.ErmError, match="Y must be 0/1 at every observed cell") as e:
            call(yb, lp)
        assert _code(e) == -1                                                              # ERM_ERR_ARG
        if logT is not None:
            tb = lp.copy(); tb[i, j] = np.nan
            with pytest.raises(L.ErmError, match="NaN in logT at an observed cell") as e:
                call(Yp, tb)
            assert _code(e) == -4                                                          # ERM_ERR_NONFINITE
            with pytest.raises(L.ErmError, match="NaN in logT") as e:                      # the NaN goes before the bad Y, as in the complete validation
                call(yb, tb)
            assert _code(e) == -4


# ------------------------------------------------------------------------------------------------------------ 6. independence
@pytest.mark.parametrize("model", ["rtirt", "cross", "mlirt"])
def test_a_subjects_result_depends_on_its_own_cells_only(model, monkeypatch):
    L, code = _pkg()._lib, mu.CODE[model]
    N, K = 33, 5
    Y, logT, X, rows, obs = ou.problem(model, N, 9, 3, seed=600)
    sl = lambda a, s: None if a is None else a[s]
    keys_ls = ["l"] + [f"{w}.{c}" for w in WEIGHTINGS for c in SCORE_KEYS]
    keys_pv = [f"pv.{c}" for c in PV_KEYS]
    whole = _products(L, code, Y, logT, X, rows, obs=obs, K=K)
    for i in (0, 5, 10, 32):                                                               # all, random, alternating, and the lone subject of the second tile
        s = slice(i, i + 1)
        alone = _products(L, code, Y[s], sl(logT, s), sl(X, s), rows, obs=obs[s], K=K)
        assert _same(alone, _at(whole, i, keys_ls), keys_ls)                               # alone (the draws: below, at the same index)
        perm = np.roll(np.arange(N), 7)                                                    # subject i at position (i + 7) mod 33
        moved = _products(L, code, Y[perm], sl(logT, perm), sl(X, perm), rows, obs=obs[perm], K=K)
        at = (i + 7) % N
        assert _same(_at(moved, at, keys_ls), _at(whole, i, keys_ls), keys_ls)
        others = np.arange(N)[::-1].copy(); others[i] = i                                  # the same index i among other subjects
        mixed = _products(L, code, Y[others], sl(logT, others), sl(X, others), rows, obs=obs[others], K=K)
        assert _same(_at(mixed, i, keys_ls + keys_pv), _at(whole, i, keys_ls + keys_pv), keys_ls + keys_pv)
    alone0 = _products(L, code, Y[:1], sl(logT, slice(0, 1)), sl(X, slice(0, 1)), rows, obs=obs[:1], K=K)
    assert _same(alone0, _at(whole, 0, keys_pv), keys_pv)                                  # index 0 alone: its draws as well
    flipped = obs.copy(); flipped[1:] = 1 - flipped[1:]                                    # every other subject's mask changes
    other = _products(L, code, Y, logT, X, rows, obs=flipped, K=K)
    assert _same(_at(other, 0, whole.keys()), _at(whole, 0, whole.keys()), whole.keys())
    assert not np.array_equal(other["l"][1], whole["l"][1])
    monkeypatch.setenv("ERM_PV_CHUNK", "5")                                                # six chunks of five and one of three: offsets past the first chunk
    chunked = L.plausible_values(code, Y, logT, X, rows, K=K, seed=11, obs=obs)
    monkeypatch.delenv("ERM_PV_CHUNK")
    assert all(np.array_equal(chunked[c], whole[f"pv.{c}"], equal_nan=True) for c in PV_KEYS) and np.array_equal(chunked["nObs"], obs.sum(axis=1))


# ------------------------------------------------------------------------------------------------------------ 7. PSIS-LOO on the masked l
def test_psis_loo_takes_the_masked_loglik():
    pkg = _pkg()
    Y, logT, X, rows, obs = ou.problem("rtirt", 33, 9, 30, seed=700)
    m = pkg._lib.marginal_loglik(1, Y, logT, X, rows, obs=obs)
    dev = pkg._lib.psis_loo(m["l"])
    host = pkg.psisLooHost(pkg.marginalLogLikHost(1, Y, logT, X, rows, 61, obs=obs))
    tol = ps.bound(ps.S_GPU) + 1e-10                                                       # tests/test_gpu_psis_loo.py: _bound() + MARGINAL_TOL
    errs = {k: ps.rel(dev[k], getattr(host, k)) for k in ("elpd_u", "p_u", "khat", "nEff")}
    errs.update({k: ps.rel([dev[k]], [getattr(host, k)]) for k in ("elpd", "pLoo", "LOOIC", "se", "lppd")})
    print("masked l through erm_psis_loo: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f"; bound {tol:.3g}")
    assert np.array_equal(np.isposinf(dev["khat"]), np.isposinf(host.khat)) and not np.any(np.isnan(dev["khat"]))
    assert all(dev[k] == getattr(host, k) for k in ("nUnits", "nRows", "nBadK", "nHighK", "tailLen")) and dev["nUnits"] == 33 and dev["nRows"] == 30
    assert all(v <= tol for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    L = _pkg()._lib
    lib = L.load()
    err = lambda: lib.erm_last_error().decode()
    N, J, F, R = 5, 9, 3, 3
    Y, logT, X, rows, obs = ou.problem("rtirt", N, J, R, seed=800)
    for bad_model, width in ((L.MODEL_CROSSQR, 5 * J + 4), (L.MODEL_LATENTQR, 4 * J + F + 2 + 4)):
        for call in (L.marginal_loglik, L.score, L.plausible_values):
            with pytest.raises(L.ErmError, match="five models without quantile weights") as e:
                call(bad_model, Y, logT, X if bad_model == L.MODEL_LATENTQR else None, np.zeros((R, width)), obs=obs)
            assert _code(e) == -1
    two = obs.copy(); two[3, 2] = 2
    for call in (L.marginal_loglik, L.score, L.plausible_values):
        with pytest.raises(L.ErmError, match=r"obs must be 0/1 \(subject 3, item 2\)") as e:
            call(1, Y, logT, X, rows, obs=two)
        assert _code(e) == -1
        with pytest.raises(L.ErmError, match="NaN in X") as e:
            xb = X.copy(); xb[4, 0] = np.nan
            call(1, Y, logT, xb, rows, obs=obs)
        assert _code(e) == -4
        with pytest.raises(L.ErmError, match="row 2: sig2t") as e:
            bad = rows.copy(); bad[2, 3 * J + 1] = 0.0
            call(1, Y, logT, X, bad, obs=obs)
        assert _code(e) == -1
    Yf, lf, Xf, Of = (np.asfortranarray(a) for a in (Y, logT, X, obs))
    p = lambda a: a.ctypes.data
    sc, o4, nn = np.zeros((7, N)), np.zeros(4), np.zeros(N, dtype=np.int32)
    raw = lambda Yp=p(Yf), lp=p(lf), Xp=p(Xf), rp=p(rows), n=N, j=J, Q=61, w=0, out=p(sc): lib.erm_score_masked(0, 1, n, j, F, Yp, lp, Xp, p(Of), rp, R, Q, w, out, p(o4), p(nn))
    assert raw(Yp=None) == -1 and "NULL" in err() and raw(rp=None) == -1 and "NULL" in err() and raw(out=None) == -1 and "NULL" in err()
    assert raw(lp=None) == -1 and "logT is required" in err() and raw(Xp=None) == -1 and "X is required" in err()
    assert raw(j=0) == -1 and "out of range" in err() and raw(j=897) == -1 and raw(n=0) == -1
    assert raw(Q=60) == -1 and "odd" in err() and raw(w=2) == -1 and "weighting" in err()
    l5, pv = np.zeros((N, R), order="F"), np.zeros((2, 5, N))
    assert lib.erm_marginal_loglik_masked(0, 1, N, J, F, p(Yf), p(lf), p(Xf), p(Of), p(rows), 1, 61, p(l5), p(o4), None, None, None) == -1 and "n_rows" in err()
    assert lib.erm_plausible_values_masked(0, 1, N, J, F, p(Yf), p(lf), p(Xf), p(Of), p(rows), R, 61, 0, 11, p(pv), None, None, None, None) == -1
    assert lib.erm_plausible_values_masked(0, 1, N, J, F, p(Yf), p(lf), p(Xf), p(Of), p(rows), R, 61, 5, 11, None, None, None, None, None) == -1
    assert raw() == 0 and list(o4[:3]) == [N, R, 61] and np.array_equal(nn, obs.sum(axis=1)) and np.all(np.isfinite(sc))      # and the device runs on


# ------------------------------------------------------------------------------------------------------------ 9. end to end
def test_masked_scores_of_a_fitted_sample_stay_near_the_complete_scores():
    """GibbsRtIrt on parity_util.make_problem("rtirt", 96, 12, 3, seed=7), 80 sweeps (40 post-burn-in rows) on the device; then the same respondents with a random
    half of their cells masked (rng 107).  Every theta must lie within 4 of its own thetaSd of the complete-data score, and the mean thetaSd must be larger.  The
    seed was chosen so that the twin alone satisfies this on the CPU with the oracle's chain of the same inputs: largest |difference| / thetaSd 1.82, mean thetaSd
    0.663 complete against 0.782 masked (seeds 8 and 9: 1.67 and 1.36)."""
    pkg = _pkg()
    N, J, F = 96, 12, 3
    Y, logT, X, init, _ = pu.make_problem("rtirt", N, J, F, seed=7)
    eng = _engine("rtirt", Y, logT, X, init, n_iter=80, n_burnin=40)
    eng.run(80)
    rows = eng.item_trace()[40:]
    eng.close()
    obs = (np.random.default_rng(107).uniform(size=(N, J)) < 0.5).astype(np.uint8)
    Ym, lm = np.where(obs != 0, Y, np.nan), np.where(obs != 0, logT, np.nan)               # the missing cells marked in the data
    assert np.array_equal(pkg.observedMask(Ym, lm), obs)
    full = pkg.scoreRespondents(1, Y, logT, X, rows)
    part = pkg.scoreRespondents(1, Ym, lm, X, rows, obs=pkg.observedMask(Ym, lm))
    host = pkg.scoresHost(1, Y, logT, X, rows, 61, obs=obs)
    assert all(ou.rel(getattr(part, c), getattr(host, c)) <= TOL for c in su.COLS) and np.array_equal(part.nObs, obs.sum(axis=1)) and full.nObs is None
    z = np.abs(part.theta - full.theta) / part.thetaSd
    print(f"largest |theta masked - theta complete| / thetaSd {z.max():.3f}; mean thetaSd complete {full.thetaSd.mean():.4f}, masked {part.thetaSd.mean():.4f}")
    assert z.max() <= 4.0 and part.thetaSd.mean() > full.thetaSd.mean() and part.nCoarse == 0
    pv = pkg.drawPlausibleValues(1, Ym, lm, X, rows, K=5, obs=obs)
    assert np.array_equal(pv.nObs, part.nObs) and np.all(np.isfinite(pv.theta)) and np.all(np.isfinite(pv.zeta))

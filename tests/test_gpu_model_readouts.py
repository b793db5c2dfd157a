"""Every per-model read-out of the engine on a live GPU against the table of per-model facts (csrc/erm_model.hpp, as tests/model_check.cpp prints it): state round
trip, trace / item-trace / Post.mean / diagnostics widths and the layout of GibbsRtIrtCrossQr's N x J block of nu, for every model in both precisions at
N = 5, J = 3, F = 2 -- N != J, so a transposed block cannot pass for the right one."""
import numpy as np
import pytest

import parity_util as pu
from test_model_traits import table  # noqa: F401  (the compiled table as a fixture)

# (A file of its own, not tests/test_host_api.py: that file's test_create_without_gpu_... asks torch whether a GPU is there, which initialises torch's copy of the
# HIP runtime; when that happens before the library's first HIP call -- test_host_api.py run alone -- erm_create then finds no device.)
pkg = pu.ge.load_package()

_RN, _RJ, _RF = 5, 3, 2


def _readout_engine(model, precision, n_iter, n_feat=_RF, cov2one=None):
    g = np.random.default_rng(3)
    Y = g.random((_RN, _RJ)) < 0.5
    logT = None if model == "mlirt" else g.normal(1.0, 0.3, (_RN, _RJ))
    X = g.standard_normal((_RN, n_feat)) if model in pu.X_MODELS and n_feat else None
    eng = pkg._lib.Engine(model=pu.MODELS[model], n_item=_RJ, n_subj=_RN, n_feat=n_feat, n_iter=n_iter, n_chain=1, n_burnin=1,
                          cov2one=int(model not in ("latentqr", "latent")) if cov2one is None else cov2one,
                          q_rt=0.85, seed=11, precision={"f32": 0, "f64": 1}[precision], trace_mode=1)
    eng.set_data(Y, logT, X)
    return eng, Y, logT, X


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model", sorted(pu.MODELS))
def test_every_readout_has_the_tables_width_and_layout(table, model, precision):
    """nIter = 4, nBurnin = 1, one chain, full traces at N = 5, J = 3, F = 2.  The state survives erm_set_state / erm_get_state entry by entry (exactly; the fp32 engine
    keeps theta, zeta and nu in fp32, so those are compared after that rounding); ra / rt / qr, the item trace, Post.mean and the diagnostics have the table's widths;
    GibbsRtIrtCrossQr's nu block of Post.qr row r is the column-major nu the sweep of that row started from.  (The diagnostics need four draws per half chain, which
    nIter = 4 does not have -- that refusal is checked -- so their widths are read from a second engine with nIter = 9.)"""
    L = pkg._lib
    N, J, F = _RN, _RJ, _RF
    t = table[(pu.MODELS[model], N, J, F)]
    f32 = (lambda v: v.astype(np.float32).astype(np.float64)) if precision == "f32" else (lambda v: v)
    eng, Y, logT, X = _readout_engine(model, precision, 4)
    # -- the data set back from the device.  The upload is transposed by a kernel (to_rows_kernel) and the download by the host's rows_to_cols, so a transposed
    # helper cannot cancel itself here; with it pinned, the state round trip below pins its inverse, cols_to_rows.  logT comes back as (centred value + column
    # mean): two roundings of the cell type around values of size <= 3
    eps = 2.0 ** -52 if precision == "f64" else 2.0 ** -23
    gY, gT, gX = eng.get_data()
    assert gY.shape == (N, J) and all(gY[i, j] == Y[i, j] for i in range(N) for j in range(J))
    assert (gT is None) == (logT is None) and (gX is None) == (X is None)
    if logT is not None:
        assert gT.shape == (N, J) and all(abs(gT[i, j] - logT[i, j]) <= 4 * 3.0 * eps for i in range(N) for j in range(J))
    if X is not None:
        assert gX.shape == (N, F) and all(gX[i, f] == f32(X)[i, f] for i in range(N) for f in range(F))
    # -- set_state -> get_state, distinct values in every entry (Sigp need not be a covariance here: nothing is run from this state)
    st = dict(theta=0.1 + 0.01 * np.arange(N), a=1.0 + 0.1 * np.arange(J), b=-0.5 + 0.1 * np.arange(J), sigp=np.array([1.5, 0.25, 0.375, 2.0]))
    if t["rt"]:
        st.update(zeta=-0.3 + 0.02 * np.arange(N), lambda_=2.0 + 0.1 * np.arange(J), sig2t=0.5 + 0.1 * np.arange(J))
    if t["rho"]:
        st["rho"] = 0.2 + 0.05 * np.arange(J)
    if t["nbeta"]:
        st["beta"] = 0.7 + 0.03 * np.arange(t["nbeta"])
    if t["nu_len"]:
        st["nu"] = 0.5 + 0.125 * np.arange(t["nu_len"])          # column-major for GibbsRtIrtCrossQr
    eng.set_state(**st)
    back = eng.get_state()
    for k, v in st.items():
        want = f32(v) if k in ("theta", "zeta", "nu") else v
        if k == "beta" and t["beta"] == "zero_pair":
            want = np.zeros(t["nbeta"])                          # GibbsRtIrtNull's beta is zero whatever is installed
        assert back[k].shape == v.shape and np.array_equal(back[k], want), (k, back[k], want)
    assert (back["beta"] is None) == (t["nbeta"] == 0) and (back["nu"] is None) == (t["nu_len"] == 0)
    # -- four sweeps, one erm_run each, from a proper state; the nu every sweep starts from
    init = dict(theta=st["theta"], a=np.ones(J), b=np.zeros(J), sigp=np.array([1.0, 0.0, 0.0, 1.0]))
    if t["rt"]:
        init.update(zeta=st["zeta"], lambda_=np.ones(J), sig2t=np.ones(J))
    for k in ("rho", "beta", "nu"):
        if k in st:
            init[k] = st[k]
    eng.set_state(**init)
    nu_before = []
    for _ in range(4):
        nu_before.append(eng.get_state(which=("nu",))["nu"])
        eng.run(1)
    ra, rt, qr = eng.trace(L.TRACE_RA), eng.trace(L.TRACE_RT), eng.trace(L.TRACE_QR)
    assert ra.shape == (4, t["ra"], 1) and qr.shape == (4, t["qr"], 1)
    assert rt.shape == ((4, t["rtw"], 1) if t["rt"] else (0,))
    assert eng.trace(L.TRACE_LOGLIKE).shape == (4, 1, 1) and eng.item_trace().shape == (4, t["item"])
    m = eng.get_mean()
    sizes = dict(theta=N, a=J, b=J, zeta=N, lambda_=J, sig2t=J, beta=t["nbeta"], sigp=4, rho=J, nu=t["nu_len"])
    assert {k: (0 if v is None else v.size) for k, v in m.items()} == sizes
    q = t["qr"] - t["nu_len"]
    if t["nu"] == "cell":
        for r in range(1, 4):          # (row 0 starts from the nu the first erm_run's prologue draws, not from the installed one)
            assert np.array_equal(qr[r, q:, 0].reshape(N, J, order="F"), nu_before[r].reshape(N, J, order="F")), r
        assert np.allclose(m["nu"], qr[1:, q:, 0].mean(axis=0), rtol=1e-12, atol=0)          # Post.mean's nu in the same layout
    if t["nu"] == "subject":
        for r in range(1, 4):
            assert np.array_equal(qr[r, q:, 0], nu_before[r]), r
    # -- diagnostics
    with pytest.raises(L.ErmError, match="too few post-burn-in iterations"):
        eng.diagnostics(L.TRACE_RA)
    eng.close()
    eng = _readout_engine(model, precision, 9)[0]
    eng.set_state(**init)
    eng.run(9)
    for which, key in ((L.TRACE_RA, "ra"), (L.TRACE_RT, "rtw"), (L.TRACE_QR, "qr")):
        if t[key] == 0:
            continue
        ess, rhat = eng.diagnostics(which)
        assert ess.shape == rhat.shape == (t[key],)
    eng.close()


# What Post.qr is made of at N = 5, J = 3, written out per (model, F) and derived from no table: (source, first column, columns) in order, where an item-trace row is
# [a 0:3 | b 3:6 | lambda 6:9 | sig2t 9:12 | the kernels' small part of qr 12:].  GibbsRtIrtNull's kernels see no covariates and publish [beta_theta0, beta_zeta0]
# at 12:14 and vec(Sigp) at 14:18 whatever F is; its Post.qr starts with 2 (F + 1) zeros that are stored nowhere.
_QR_CONTENT = {
    ("mlirt", 2): [("item", 12, 3)],                                        # beta (F + 1)
    ("rtirt", 2): [("item", 12, 6), ("item", 18, 4)],                       # vec(beta) (2 (F + 1)), vec(Sigp)
    ("null", 2): [("zero", 0, 6), ("item", 14, 4)],
    ("null", 0): [("zero", 0, 2), ("item", 14, 4)],
    ("cross", 2): [("item", 12, 3), ("item", 15, 4)],                       # rho (J), vec(Sigp)
    ("crossqr", 2): [("item", 12, 3), ("item", 15, 4), ("nu", 0, 15)],      # ..., vec(nu) (N J)
    ("latent", 2): [("item", 12, 4), ("item", 16, 4)],                      # beta (F + 2), vec(Sigp)
    ("latentqr", 2): [("item", 12, 4), ("item", 16, 4), ("nu", 0, 5)],      # ..., nu (N)
}
_ITEM_WIDTH = {("mlirt", 2): 15, ("rtirt", 2): 22, ("null", 2): 18, ("null", 0): 18, ("cross", 2): 19, ("crossqr", 2): 19, ("latent", 2): 20, ("latentqr", 2): 20}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("model,F", sorted(_QR_CONTENT))
def test_every_trace_column_holds_what_its_name_says(model, F, precision):
    """erm_get_trace and the diagnostics read one list of blocks, so comparing one with the other cannot notice a list that is wrong; this pins the CONTENTS against
    read-outs that do not go through it.  nIter = 4, one chain, full traces, one erm_run per row: row r of Post.ra starts with the theta erm_get_state returns after
    that run and goes on with columns a, b of the item trace; Post.rt the same with zeta, lambda, sig2t; Post.qr is the literal map above (its nu block is pinned by
    test_every_readout_has_the_tables_width_and_layout).  All exact.  Then, for GibbsRtIrtNull at nIter = 9 with all four entries of Sigp drawn, the NaN entries
    of the diagnostics of Post.qr are exactly its zero columns."""
    L = pkg._lib
    N, J = _RN, _RJ
    start = dict(theta=0.1 + 0.01 * np.arange(N)) if model == "mlirt" else dict(theta=0.1 + 0.01 * np.arange(N), zeta=-0.3 + 0.02 * np.arange(N))
    eng = _readout_engine(model, precision, 4, F)[0]
    eng.set_state(**start)          # (subjects that all start at zero leave the latent regression of zeta on theta nothing to estimate)
    theta, zeta = [], []
    for _ in range(4):
        eng.run(1)
        st = eng.get_state(which=("theta", "zeta"))
        theta.append(st["theta"])
        zeta.append(st["zeta"])
    item = eng.item_trace()
    assert item.shape == (4, _ITEM_WIDTH[model, F]) and np.all(np.isfinite(item))
    ra = eng.trace(L.TRACE_RA)[:, :, 0]
    assert ra.shape == (4, N + 2 * J)
    assert np.array_equal(ra[:, :N], np.array(theta)) and len({tuple(v) for v in theta}) == 4
    assert np.array_equal(ra[:, N:N + J], item[:, 0:J]) and np.array_equal(ra[:, N + J:], item[:, J:2 * J])
    if model == "mlirt":
        assert eng.trace(L.TRACE_RT).size == 0
    else:
        rt = eng.trace(L.TRACE_RT)[:, :, 0]
        assert rt.shape == (4, N + 2 * J)
        assert np.array_equal(rt[:, :N], np.array(zeta)) and len({tuple(v) for v in zeta}) == 4
        assert np.array_equal(rt[:, N:N + J], item[:, 2 * J:3 * J]) and np.array_equal(rt[:, N + J:], item[:, 3 * J:4 * J])
    qr = eng.trace(L.TRACE_QR)[:, :, 0]
    content = _QR_CONTENT[model, F]
    assert qr.shape == (4, sum(n for _, _, n in content))
    col = 0
    for source, first, n in content:
        if source == "item":
            assert np.array_equal(qr[:, col:col + n], item[:, first:first + n]), (source, first, n)
        elif source == "zero":
            assert np.all(qr[:, col:col + n] == 0.0)
        col += n
    if model == "null":
        assert np.all(qr[:, :2 * (F + 1)] == 0.0) and np.array_equal(qr[:, -4:], item[:, -4:]) and qr.shape[1] == 2 * (F + 1) + 4
    # the item-level draws are all different from one another in every row, so a shifted or swapped item block cannot pass for the right one
    drawn = 2 * J if model == "mlirt" else 4 * J
    assert all(len(set(row[:drawn])) == drawn for row in item)
    eng.close()
    if model == "null":
        eng = _readout_engine(model, precision, 9, F, cov2one=0)[0]          # (cov2one would pin Sigp's diagonal at 1: two more constant columns)
        eng.set_state(**start)
        eng.run(9)
        ess, rhat = eng.diagnostics(L.TRACE_QR)
        zero = np.arange(2 * (F + 1) + 4) < 2 * (F + 1)
        assert np.array_equal(np.isnan(ess), zero) and np.array_equal(np.isnan(rhat), zero)
        eng.close()

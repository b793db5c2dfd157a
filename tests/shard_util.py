"""Helpers of the subject-sharding tests (test_gpu_sharded.py, test_gpu_sharded_regimes.py): shards of one chain as engines of this process on the one
GPU, driven by host threads (parallel.run_sharded_threads), their traces put back together in the layout of the unsharded chain, and the fp64 CPU oracle
on the UNSHARDED data.  Test infrastructure only."""
import numpy as np

import __graft_entry__ as ge
import parity_util as pu
from parity_util import MODELS


def engine_state(init):
    """make_problem's initial state under the keyword names of Engine.set_state."""
    return {("lambda_" if k == "lam" else k): v for k, v in init.items()}


def cov2one_of(model):
    return model not in ("latentqr", "latent")


def run_shards(model, Y, logT, X, init, nsweeps, count, *, rows=None, precision="f64", seed=1234, qRt=0.85, n_chain=1, n_burnin=None, trace_mode=1,
               script=None, **opts):
    """`count` shards of one chain on (Y, logT, X) from `init`: (engines, rows).  nsweeps sweeps are dealt to n_chain trace slabs as the unsharded engine
    deals them (n_iter = nsweeps / n_chain); `script(rank, engine)` replaces the single run(nsweeps)."""
    pkg = ge.load_package()
    L = pkg._lib
    N, J = Y.shape
    Fx = 0 if X is None else X.shape[1]
    assert nsweeps % n_chain == 0
    nb = (nsweeps // n_chain) // 2 if n_burnin is None else n_burnin

    def make_engine(n_local):
        return L.Engine(model=MODELS[model], n_item=J, n_subj=n_local, n_feat=Fx, n_iter=nsweeps // n_chain, n_chain=n_chain, n_burnin=nb,
                        cov2one=int(cov2one_of(model)), q_rt=qRt, seed=seed, precision={"f32": 0, "f64": 1}[precision], trace_mode=trace_mode, **opts)

    engines = pkg.parallel.run_sharded_threads(make_engine, count, N, Y, logT, X, engine_state(init), nsweeps, rows=rows, script=script)
    return engines, (pkg.parallel.shard_rows(N, count) if rows is None else [tuple(r) for r in rows])


def concat_traces(model, engines, rows, J, Fx):
    """The shards' FULL traces as the unsharded chain's: {dev_ra, dev_rt, dev_qr, dev_ll}, rows x width in the order the sweeps ran.  Subject blocks
    concatenate over the shards; item and structural blocks and the log-likelihood must be identical on every shard, bit for bit (asserted)."""
    L = ge.load_package()._lib
    count = len(engines)
    N = sum(n for _, n in rows)
    out = {}
    for name, which in (("ra", L.TRACE_RA),) + ((("rt", L.TRACE_RT),) if model != "mlirt" else ()):
        tr = [pu.trace_rows(e.trace(which)) for e in engines]
        for r in range(1, count):
            np.testing.assert_array_equal(tr[r][:, rows[r][1]:], tr[0][:, rows[0][1]:])
        out["dev_" + name] = np.concatenate([tr[r][:, :rows[r][1]] for r in range(count)] + [tr[0][:, rows[0][1]:]], axis=1)
    qr = [pu.trace_rows(e.trace(L.TRACE_QR)) for e in engines]
    T = qr[0].shape[0]
    k = {"latentqr": Fx + 2 + 4, "crossqr": J + 4}.get(model, qr[0].shape[1])
    for r in range(1, count):
        np.testing.assert_array_equal(qr[r][:, :k], qr[0][:, :k])
    if model == "latentqr":
        out["dev_qr"] = np.concatenate([qr[0][:, :k]] + [qr[r][:, k:] for r in range(count)], axis=1)
    elif model == "crossqr":
        nus = [qr[r][:, k:].reshape(T, rows[r][1], J, order="F") for r in range(count)]       # vec(nu) is column-major [n_local x J]
        out["dev_qr"] = np.concatenate([qr[0][:, :k], np.concatenate(nus, axis=1).reshape(T, N * J, order="F")], axis=1)
    else:
        out["dev_qr"] = qr[0]
    ll = [pu.trace_rows(e.trace(L.TRACE_LOGLIKE))[:, 0] for e in engines]
    for r in range(1, count):
        np.testing.assert_array_equal(ll[r], ll[0])
    out["dev_ll"] = ll[0]
    return out


def oracle_chain(model, Y, logT, X, init, nsweeps, *, seed=1234, qRt=0.85, threads=1):
    """The fp64 CPU oracle's unsharded chain on the same inputs: {ra, rt, qr, ll}."""
    with pu.oracle_threads(threads):
        op = pu.OracleProblem(model, Y, logT, X, init, qRt=qRt, cov2one=cov2one_of(model), seed=seed)
        return op.run(nsweeps, with_nu=model in pu.NU_MODELS)


def sharded_result(model, Y, logT, X, init, nsweeps, count, *, orc=None, oracle_threads=1, **kw):
    """run_shards + concat_traces + the oracle (or `orc`, a chain computed before on the same inputs), in the shape pu.max_rel_err reads."""
    engines, rows = run_shards(model, Y, logT, X, init, nsweeps, count, **kw)
    res = concat_traces(model, engines, rows, Y.shape[1], 0 if X is None else X.shape[1])
    if orc is None:
        orc = oracle_chain(model, Y, logT, X, init, nsweeps, seed=kw.get("seed", 1234), qRt=kw.get("qRt", 0.85), threads=oracle_threads)
    res.update(orc=orc, model=model, engines=engines, rows=rows)
    return res


def sharded(model, N, J, nsweeps, count, *, F=3, precision="f64", seed=7, qRt=0.85, **opts):
    """`count` near-equal shards of make_problem(model, N, J) against the oracle's unsharded chain."""
    Y, logT, X, init, _ = pu.make_problem(model, N, J, F, seed=seed, qRt=qRt)
    return sharded_result(model, Y, logT, X, init, nsweeps, count, precision=precision, qRt=qRt, **opts)


def split_state(state, n_total, lo, n):
    """The rows [lo, lo + n) of a whole-chain state (Engine.set_state keywords): theta, zeta and vec(nu) are cut, the rest is shared."""
    st = dict(state)
    for k in ("theta", "zeta"):
        if st.get(k) is not None:
            st[k] = np.ascontiguousarray(np.asarray(st[k])[lo:lo + n])
    if st.get("nu") is not None:
        st["nu"] = np.asfortranarray(np.asarray(st["nu"]).reshape(n_total, -1, order="F")[lo:lo + n]).reshape(-1, order="F")
    return st


def snapshot(eng, model, full=True):
    """Everything an engine reports about its chain, for bit-for-bit comparisons: traces (FULL engines), item trace, logLike, Post.mean, post_count, state."""
    L = ge.load_package()._lib
    out = {"item": eng.item_trace(), "ll": eng.trace(L.TRACE_LOGLIKE), "post_count": np.array(eng.post_count)}
    if full:
        out["ra"], out["qr"] = eng.trace(L.TRACE_RA), eng.trace(L.TRACE_QR)
        if model != "mlirt":
            out["rt"] = eng.trace(L.TRACE_RT)
    for tag, d in (("mean_", eng.get_mean()), ("state_", eng.get_state())):
        out.update({tag + k: v for k, v in d.items() if v is not None})
    return out


def assert_same_bits(a, b, label, skip=()):
    assert set(a) == set(b), (label, sorted(set(a) ^ set(b)))
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k], equal_nan=True), (label, k, float(np.nanmax(np.abs(np.asarray(a[k], dtype=float) - np.asarray(b[k], dtype=float)))))

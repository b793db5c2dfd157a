"""An independent reference for the rank-normalised convergence diagnostics (erm_get_rank_diagnostics / erm_debug_rank_diagnostics, twins.rank_ess_rhat): bulk-ESS,
tail-ESS and rank-normalised split-R-hat of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), written from the definition in include/ertirt.h -- nothing is
imported from the package.  The transforms are numpy / scipy; the estimator behind them is diag_util.reference, the long-double one.

The definition.  The used draws of a column are diag_util's: the first and last n = floor(Tn / 2) post-burn-in draws of every chain, M = 2 C sequences, S = M n
pooled draws.  E(.) and R(.) are diag_util's ess and rhat of a transformed column.
    r_i  = scipy.stats.rankdata(pooled used draws, method="average")
    z_i  = ndtri((r_i - 3/8) / (S + 1/4))                                  ess_bulk = E(z)
    med  = (x_(S/2) + x_(S/2+1)) / 2,  f_i = |x_i - med|,  z' = z(f)        rhat_rank = max(R(z), R(z')) over those that are defined
    k    = (S + 19) // 20,  L_i = [x_i <= x_(k)],  U_i = [x_i >= x_(S+1-k)]  ess_tail = min(E(L), E(U)), NaN if either indicator is constant
A column that never moves has three NaN."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

import diag_util as du

ESS_RTOL, RHAT_ATOL, MARGIN_MIN, SKIP_CAP = du.ESS_RTOL, du.RHAT_ATOL, du.MARGIN_MIN, du.SKIP_CAP
SERIES = ("z", "zf", "L", "U")


def used(x):
    """x[iteration, column, chain] -> the used draws [2 n, column, chain] (an odd length drops the middle draw)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("x must be [iteration, column, chain]")
    Tn = x.shape[0]
    n = Tn // 2
    return np.concatenate([x[:n], x[Tn - n:]], axis=0)


def _scores(u):
    """normal scores of the pooled average ranks, per column: u[draw, column, chain] -> the same shape"""
    T2, K, C = u.shape
    S = T2 * C
    flat = u.transpose(0, 2, 1).reshape(S, K)
    r = rankdata(flat, method="average", axis=0)
    z = ndtri((r - 0.375) / (S + 0.25))
    return z.reshape(T2, C, K).transpose(0, 2, 1)


def transforms(x):
    """The four series of the definition for every column of x[iteration, column, chain], each [2 n, column, chain]: z, zf (the scores of the folded draws), L, U."""
    u = used(x)
    T2, K, C = u.shape
    S = T2 * C
    srt = np.sort(u.transpose(0, 2, 1).reshape(S, K), axis=0)
    k = (S + 19) // 20
    med = 0.5 * (srt[S // 2 - 1] + srt[S // 2])
    return dict(z=_scores(u), zf=_scores(np.abs(u - med[None, :, None])), L=(u <= srt[k - 1][None, :, None]).astype(np.float64),
                U=(u >= srt[S - k][None, :, None]).astype(np.float64), S=S, k=k)


def reference(x):
    """x[iteration, column, chain] -> dict(ess_bulk, ess_tail, rhat_rank: np.longdouble per column; rz, rf: the two R-hats; constant: the column never moves;
    margin: the smallest stop-rule margin over the column's four series (diag_util.reference); fold_wins: R(z') > R(z))."""
    t = transforms(x)
    ref = {s: du.reference(t[s]) for s in SERIES}
    rz, rf = ref["z"]["rhat"], ref["zf"]["rhat"]
    el, eu = ref["L"]["ess"], ref["U"]["ess"]
    nan = np.longdouble("nan")
    with np.errstate(invalid="ignore"):
        tail = np.where(np.isnan(el) | np.isnan(eu), nan, np.minimum(el, eu))
        fold_wins = rf > rz
    margin = np.min(np.stack([ref[s]["margin"] for s in SERIES]), axis=0)
    return dict(ess_bulk=ref["z"]["ess"], ess_tail=tail, rhat_rank=np.fmax(rz, rf), rz=rz, rf=rf, constant=ref["z"]["constant"], margin=margin,
                fold_wins=fold_wins, S=t["S"], k=t["k"])


def compare(bulk, tail, rhat, ref, *, ess_rtol=ESS_RTOL, rhat_atol=RHAT_ATOL, margin_min=MARGIN_MIN):
    """An estimator's three vectors against reference(x).  The NaN pattern must match exactly in all three; columns whose stop rule was decided by less than
    `margin_min` in any of the four series are left out of the value comparison and counted.  Returns dict(bulk_err, tail_err: worst relative errors, rhat_err: worst
    absolute error, skipped, compared, bad: indices of the columns that miss a tolerance or the NaN pattern)."""
    got = [np.asarray(v, dtype=np.float64) for v in (bulk, tail, rhat)]
    want = [ref["ess_bulk"], ref["ess_tail"], ref["rhat_rank"]]
    K = want[0].shape[0]
    nan_ok = np.ones(K, dtype=bool)
    for g, w in zip(got, want):
        if g.shape != (K,):
            raise ValueError(f"{g.shape} values for {K} columns")
        nan_ok &= np.isnan(g) == np.isnan(w.astype(np.float64))
    use = ref["margin"] >= margin_min
    errs = []
    ok = np.ones(K, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for q, (g, w) in enumerate(zip(got, want)):
            live = use & ~np.isnan(w.astype(np.float64))
            d = np.abs(g.astype(np.longdouble) - w)
            e = np.where(live, d / np.abs(w) if q < 2 else d, 0).astype(np.float64)
            errs.append(float(e.max(initial=0.0)))
            ok &= ~live | (e <= (ess_rtol if q < 2 else rhat_atol))
    return dict(bulk_err=errs[0], tail_err=errs[1], rhat_err=errs[2], skipped=int(np.sum(~use & ~ref["constant"])), compared=int(np.sum(use & ~ref["constant"])),
                bad=np.flatnonzero(~nan_ok | ~ok))


def counts6(bulk, tail, rhat, ess_min=400.0, rhat_max=1.1):
    """erm_get_rank_convergence's six counts from the vectors."""
    b, t, r = (np.asarray(v, dtype=np.float64) for v in (bulk, tail, rhat))
    with np.errstate(invalid="ignore"):
        return (int(np.sum(~np.isnan(b))), int(np.sum(b > ess_min)), int(np.sum(~np.isnan(t))), int(np.sum(t > ess_min)),
                int(np.sum(~np.isnan(r))), int(np.sum(r < rhat_max)))


# the shapes at which each mechanism of the device kernel can go wrong: S = 8 (k = 1), a short power of two, an odd length, S = 78 (no power of two), two
# workgroup-strides, several draws per lane, M = 32 sequences
PAIRS = ((8, 1), (16, 1), (17, 2), (27, 3), (64, 2), (200, 4), (40, 16))
NCOLS = (1, 63, 65, 193)
KINDS = 6


def synthetic(n_draw, n_chain, n_col, seed):
    """x[n_draw, n_col, n_chain], column k of kind k mod 6:
    0 AR(1) with phi in (-0.5, 0.95); 1 Cauchy with the last chain shifted by 2; 2 equal location, chain scales 1, 3, 5, ... (a single chain: its second half
    scaled by 3); 3 floor(2 x) of an AR(1): heavy ties; 4 float-rounded values at an offset of 1000 (ties after rounding); 5 exp(3 x): skewed, heavy right tail."""
    rng = np.random.default_rng(seed)
    x = np.empty((n_draw, n_col, n_chain))

    def ar1(phi):
        e = rng.standard_normal((n_draw, n_chain))
        out = np.empty_like(e)
        out[0] = e[0]
        for m in range(1, n_draw):
            out[m] = phi * out[m - 1] + np.sqrt(1 - phi * phi) * e[m]
        return out

    for k in range(n_col):
        kind = k % KINDS
        phi = rng.uniform(-0.5, 0.95)
        if kind == 0:
            v = ar1(phi)
        elif kind == 1:
            v = rng.standard_cauchy((n_draw, n_chain))
            v[:, -1] += 2.0
            if n_chain == 1:
                v[n_draw // 2:, 0] += 2.0
        elif kind == 2:
            v = rng.standard_normal((n_draw, n_chain)) * (1.0 + 2.0 * np.arange(n_chain))[None, :]
            if n_chain == 1:
                v[n_draw // 2:, 0] *= 3.0
        elif kind == 3:
            v = np.floor(2.0 * ar1(phi))
        elif kind == 4:
            v = (1000.0 + 0.01 * ar1(phi)).astype(np.float32).astype(np.float64)
        else:
            v = np.exp(3.0 * ar1(phi))
        x[:, k, :] = v
    return x


def edge_columns(n_draw, n_chain):
    """x[n_draw, 6, n_chain]: constant; two-valued and evenly split (f constant: R(z') undefined); all ties but one; -0.0 / +0.0 mixed with +-1; +-inf among
    normals; a ramp."""
    rng = np.random.default_rng(7)
    x = np.empty((n_draw, 6, n_chain))
    x[:, 0, :] = 0.1
    two = np.where(rng.permutation(n_draw * n_chain) % 2 == 0, 1.5, -0.5).reshape(n_draw, n_chain)
    x[:, 1, :] = two
    x[:, 2, :] = 3.0
    x[1, 2, 0] = 7.0
    z = rng.integers(0, 4, (n_draw, n_chain))
    x[:, 3, :] = np.choose(z, [-0.0, 0.0, 1.0, -1.0])
    v = rng.standard_normal((n_draw, n_chain))
    v[0, 0], v[-1, -1] = np.inf, -np.inf
    x[:, 4, :] = v
    x[:, 5, :] = (np.arange(n_draw)[:, None] * n_chain + np.arange(n_chain)[None, :]) * 0.25
    return x

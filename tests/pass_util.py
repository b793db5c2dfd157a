"""Helpers shared by the tests of the passes behind a sweep at the edges of their launch geometry and on extreme data (tests/test_pass_geometry_host.py,
tests/test_gpu_pass_geometry.py, tests/test_gpu_pass_extremes.py).

 1. pass_geom(): the Python side of erm_geometry.hpp's pass_geom -- restated here from the header, and held to it case by case and on a grid by the host test
    through tests/pass_geom_check.cpp -- so that a GPU test can ask, with the card's compute-unit count, what the engine will launch.
 2. The table of GPU cases, each with the regime its id claims as PROPERTIES OF THE PLAN (regime_misses): a case that drifts out of its regime when a constant of
    the kernels moves fails on the CPU instead of quietly testing something else.
 3. The extended-precision reference of the cell arithmetic (np.longdouble, 64-bit significand) with the condition sum of every unit beside its value, the
    rounding bounds derived from it, and the constants c measured for the fp64 numpy twins on the oracle chain (EXTREME_C).
Test infrastructure only: nothing here is imported by the package."""
from __future__ import annotations

import collections
import functools

import numpy as np

import parity_util as pu
import ppc_util as ppu
import waic_util as wu

MODELS = list(ppu.MODELS)
CHAIN = dict(n_iter=4, n_burnin=1)          # 3 post-burn-in rows, 3 replicates (thin 1): WAIC needs two rows
LDS_LIMIT = 160 * 1024
PASS_THREADS, PRED_MAX_BLOCKS, PRED_IT_PARTS = 256, 1024, 16


# ----------------------------------------------------------------------------------------------------------------- 1. the plan
def pass_log_lanes(J):
    lw = 0
    while (1 << lw) < 64 and (4 << lw) < J:
        lw += 1
    return lw


def pred_lds_bytes(model, J, T, logW):
    return (6 * J + (T >> logW) * (3 if model == "mlirt" else 5) * J) * 8


def pass_geom(model, N, J, cu_count):
    """erm_geometry.hpp, pass_geom: {logW, T, R, nq, nb_pred, lds_pred, R_pw, nb_pw_subject, nb_pw_cell, lds_pw, nb_loglik, rows_per_block, lds_loglik}."""
    logW, T = pass_log_lanes(J), PASS_THREADS
    while T > 64 and pred_lds_bytes(model, J, T, logW) > LDS_LIMIT:
        T >>= 1
    R, R_pw = T >> logW, PASS_THREADS >> logW
    nb_ll = min(1024, (N + 63) // 64)
    return dict(logW=logW, T=T, R=R, nq=3 if model == "mlirt" else 5, nb_pred=min(-(-N // R), PRED_MAX_BLOCKS), lds_pred=pred_lds_bytes(model, J, T, logW), R_pw=R_pw,
                nb_pw_subject=min(-(-N // R_pw), cu_count * 8), nb_pw_cell=min(-(-(N * J) // PASS_THREADS), cu_count * 16), lds_pw=7 * J * 8, nb_loglik=nb_ll,
                rows_per_block=-(-N // nb_ll), lds_loglik=(5 * J + 4 + 2 * 16) * 8)


# ----------------------------------------------------------------------------------------------------------------- 2. the cases
Case = collections.namedtuple("Case", "id regime model precision N J F seed")
LANES = {1: 1, 2: 1, 4: 1, 5: 2, 8: 2, 9: 4, 16: 4, 17: 8, 32: 8, 33: 16, 64: 16, 65: 32, 128: 32, 129: 64}      # J -> lanes per subject, both sides of every switch
X_SINGULAR_AT_ONE_SUBJECT = ("mlirt", "rtirt")      # regress on [1 x]: with one subject and a covariate the model itself is undefined (the host test shows the NaN)


def _R(model, J):
    return pass_geom(model, 1, J, 1)["R"]


def replicate_cases(cu_count):
    """Every case that runs WAIC (subject, then cell) and the replicate pass against the twins.  cu_count: the card's compute units (the cap cases are computed from it)."""
    out = []
    for model in MODELS:                                     # lane widths and their switches: two workgroups, the second holding one subject and R - 1 idle slots
        for precision in ("f64", "f32") if model in ("rtirt", "crossqr") else ("f64",):
            for J, W in LANES.items():
                out.append(Case(f"lanes-{model}-{precision}-J{J}-W{W}", ("lanes", W), model, precision, _R(model, J) + 1, J, 3, 17))
    for model in ("rtirt", "mlirt", "crossqr"):              # subject tails: one workgroup, N <= R
        for J in (4, 17, 129):
            R = _R(model, J)
            for what, N in (("one", 1), ("two", 2), ("R-1", R - 1), ("R", R)):
                # (one subject and one covariate: the regression on [1 x] is singular -- those two models run their N = 1 case without covariates)
                F = 0 if N == 1 and model in X_SINGULAR_AT_ONE_SUBJECT else 1
                # (two subjects whose 0/1 covariate happens to agree are singular in the same way: those seeds are the first at which the oracle chain is finite)
                seed = {("mlirt", 17, 2): 19, ("mlirt", 129, 2): 18}.get((model, J, N), 17)
                out.append(Case(f"tail-{model}-J{J}-N{what}", ("tail", what), model, "f64", N, J, F, seed))
    out.append(Case("items-rtirt-nb17", ("items", 17), "rtirt", "f64", 65, 129, 3, 17))
    out.append(Case("items-rtirt-nb1024", ("items", 1024), "rtirt", "f64", 4096, 129, 3, 17))
    for model in ("rtirt", "crossqr"):
        out.append(Case(f"cap-{model}-slab", ("cap_pred",), model, "f64", 4101, 129, 3, 17))
        out.append(Case(f"cap-{model}-waic", ("cap_waic",), model, "f64", cu_count * 8 * 4 + 5, 129, 3, 17))
    out.append(Case("lds-rtirt-J787", ("lds_edge", 256), "rtirt", "f64", 2 * _R("rtirt", 787) + 1, 787, 3, 17))
    out.append(Case("lds-rtirt-J788", ("lds_edge", 128), "rtirt", "f64", 2 * _R("rtirt", 788) + 1, 788, 3, 17))
    out.append(Case("lds-mlirt-J896", ("lds_ra", 256), "mlirt", "f64", 2 * _R("mlirt", 896) + 1, 896, 3, 17))
    return out


def dic_cases():
    """loglik_kernel: N in {1, 63, 64, 65, 129} x J in {5, 257}, (65, 896), (129, 1); one past the grid's cap (65 537 x 1: workgroups past the end).  Without
    covariates, so that one subject is a defined model -- in all but GibbsRtIrtLatentQr, which regresses zeta on [1 theta] with a weight per subject and has no N = 1 case."""
    shapes = [(N, J) for N in (1, 63, 64, 65, 129) for J in (5, 257)] + [(65, 896), (129, 1)]
    out = [Case(f"dic-{model}-{precision}-{N}x{J}", ("dic",), model, precision, N, J, 0, 17) for model in MODELS for precision in (("f64", "f32") if model == "rtirt" else ("f64",))
           for N, J in shapes if not (N == 1 and model == "latentqr")]
    return out + [Case(f"dic-{model}-f64-65537x1", ("dic_past_end",), model, "f64", 65537, 1, 0, 17) for model in ("rtirt", "mlirt")]


def regime_misses(case, p, cu_count):
    """The properties of plan p (pass_geom's keys) that case.regime claims and p does not have."""
    N, J, kind = case.N, case.J, case.regime[0]
    W, R, Rpw = 1 << p["logW"], p["R"], p["R_pw"]
    chunks, chunks_pw = -(-N // R), -(-N // Rpw)
    if kind == "lanes":
        want = case.regime[1]
        props = [(f"{want} lanes per subject", W == want), ("at most four items per lane, or all 64 lanes", 4 * W >= J or W == 64),
                 ("J sits on a switch of the lane width (or below the first)", J <= 2 or 1 << pass_log_lanes(J + 1) == 2 * W or (W > 1 and 1 << pass_log_lanes(J - 1) == W // 2)),
                 ("two workgroups in both passes, the second holding one subject", N == R + 1 == Rpw + 1 and p["nb_pred"] == 2 and p["nb_pw_subject"] == 2)]
    elif kind == "tail":
        want = dict(one=1, two=2)
        want.update({"R-1": R - 1, "R": R})
        props = [("one workgroup in both passes", p["nb_pred"] == 1 and p["nb_pw_subject"] == 1 and R == Rpw), (f"N = {case.regime[1]}", N == want[case.regime[1]] and 1 <= N <= R)]
    elif kind == "items":
        nb, per = p["nb_pred"], -(-p["nb_pred"] // PRED_IT_PARTS)
        full, rest = divmod(nb, per)
        props = [(f"{case.regime[1]} slab rows, no second trip", nb == case.regime[1] == chunks)]
        props += [("per = 2: eight full parts, one half full, seven empty", per == 2 and full == 8 and rest == 1)] if case.regime[1] == 17 else \
                 [("the slab at its cap exactly, sixteen full parts", nb == PRED_MAX_BLOCKS and per * PRED_IT_PARTS == nb)]
    elif kind == "cap_pred":
        props = [("the slab is capped", p["nb_pred"] == PRED_MAX_BLOCKS < chunks), ("workgroups 0 and 1 take a second trip", chunks == PRED_MAX_BLOCKS + 2),
                 ("the last subject is alone in its chunk", N - (chunks - 1) * R == 1)]
    elif kind == "cap_waic":
        props = [("WAIC in subject units is past its cap", p["nb_pw_subject"] == cu_count * 8 < chunks_pw), ("WAIC in cell units is past its cap", p["nb_pw_cell"] == cu_count * 16 < -(-(N * J) // PASS_THREADS))]
    elif kind == "lds_edge":
        T = case.regime[1]
        other = pass_geom(case.model, N, J + 1 if T == 256 else J - 1, cu_count)
        props = [(f"{T} threads", p["T"] == T), ("within the LDS limit", p["lds_pred"] <= LDS_LIMIT), ("the neighbouring J is on the other side of the switch", other["T"] == (128 if T == 256 else 256)),
                 ("three chunks, the last holding one subject", N == 2 * R + 1 and p["nb_pred"] == 3)]
        if T == 256:
            props.append(("within 256 bytes of the limit", p["lds_pred"] > LDS_LIMIT - 256))
    elif kind == "lds_ra":
        props = [("256 threads at the item limit", p["T"] == 256 and J == 896 and p["nq"] == 3), ("within the LDS limit", p["lds_pred"] <= LDS_LIMIT), ("three chunks", N == 2 * R + 1 and p["nb_pred"] == 3)]
    elif kind == "dic":
        nb, rpb = p["nb_loglik"], p["rows_per_block"]
        props = [("workgroups of at most 64 subjects cover N, none of them empty", nb == -(-N // 64) and rpb <= 64 and (nb - 1) * rpb < N <= nb * rpb)]
    elif kind == "dic_past_end":
        nb, rpb = p["nb_loglik"], p["rows_per_block"]
        props = [("the grid is capped and its last workgroups start past the end", nb == 1024 and (nb - 1) * rpb >= N)]
    else:
        raise KeyError(kind)
    return [what for what, ok in props if not ok]


@functools.lru_cache(maxsize=4)
def problem(model, N, J, F, seed):
    """parity_util.make_problem; GibbsMlIrt without covariates (its generator needs one) is generated with one and fitted without."""
    if model == "mlirt" and F == 0:
        Y, logT, X, init, tp = pu.make_problem(model, N, J, 1, seed=seed)
        return Y, logT, np.zeros((N, 0), order="F"), dict(init, beta=np.asarray(init["beta"])[:1]), tp
    return pu.make_problem(model, N, J, F, seed=seed)


def oracle_sampler(case, n_iter, n_burnin, prob=None):
    """The oracle chain of a case wrapped for the twins (waic_util.oracle_sampler's defaults: qRt 0.85, seed 1234)."""
    Y, logT, X, init, _ = prob if prob is not None else problem(case.model, case.N, case.J, case.F, case.seed)
    return wu.oracle_sampler(case.model, Y, logT, None if X is None or X.shape[1] == 0 else X, init, n_iter, nBurnin=n_burnin)


def excluded_share(P):
    """(units excluded by ppc_util's margin rule, units) of a getPpcHost result."""
    ex = ppu.excluded_units(P)
    n_ex = n = 0
    for name, acc in (("item", P.item), ("subject", P.subj), ("total", P.total)):
        for c in range(acc.shape[0]):
            if np.all(np.isnan(acc[c])):
                continue
            e = np.atleast_1d(ex[name][c])
            n += e.size
            n_ex += int(e.sum())
    return n_ex, n


# ----------------------------------------------------------------------------------------------------------------- 3. extended precision
LD = np.longdouble
U53 = 2.0 ** -53
FLOOR = 2.0 ** -1022         # below fp64's smallest normal number a result has no relative precision (exp(-2 000) is 0 in fp64, 1e-869 in long double): absolute, per unit
EXTREME_CHAIN = dict(n_iter=6, n_burnin=2)      # 4 post-burn-in rows, 4 replicates
EXTREME_SHAPE = (1200, 24)
# c of `|twin - ref| <= c 2^-53 cond_u`: the largest ratio of the fp64 numpy twins (pointwiseLogLikHost, getPpcHost, getLogLikelihood) against the extended reference
# over every model of the kind and every unit sum, on the oracle chain at EXTREME_SHAPE, rounded up (tests/test_pass_geometry_host.py measures it again and holds it
# to these).  The device is granted 8 c, and at least 8: its libm may differ from numpy's by an ulp per transcendental, and it adds in another order.
# Measured (largest, where): separated 83.9 (crossqr, l of a cell), saturated 740 (mlirt, l of a cell: exp(eta) at eta ~ -740 carries the rounding of eta, |eta| 2^-53
# relative), degenerate 163 (crossqr, l of a cell), rt_offset 2 770 (crossqr, l of a cell: (logT - mu)^2 / var at var ~ 1e-4 from a residual of two numbers ~ 8),
# x_offset 11.7 (latentqr, an item's D^T_obs).
EXTREME_C = {"separated": 85.0, "saturated": 750.0, "degenerate": 165.0, "rt_offset": 2800.0, "x_offset": 12.0}


def device_c(kind):
    return max(8.0, 8.0 * EXTREME_C[kind])


def _log1pexp(x):
    return np.where(x > 0, x, LD(0)) + np.log1p(np.exp(-np.abs(x)))


class Extended:
    """The definitions of DESIGN.md 7c / 7g in np.longdouble from fp64 inputs; every value comes with the sum of the absolute values of what was added to form it (its
    condition sum).  The response term is written in the form that does not cancel: l = -log1pexp(-s eta), s = +1 for y = 1, -1 for y = 0."""

    def __init__(self, model, Y, logT, qRt=0.85):
        if np.finfo(LD).nmant < 63:
            raise RuntimeError("np.longdouble is not wider than fp64 on this platform")
        self.model, self.N, self.J = model, Y.shape[0], Y.shape[1]
        self.Y = np.asarray(Y, dtype=LD)
        self.logT = None if model == "mlirt" else np.asarray(logT, dtype=LD)
        q = LD(qRt)
        self.k1, self.k2 = ((1 - 2 * q) / (q * (1 - q)), 2 / (q * (1 - q))) if model in ("crossqr", "latentqr") else (LD(0), LD(1))

    def cells(self, th, a, b, ze=None, lam=None, sg=None, rho=None, nu=None):
        """One parameter point -> dict of (N, J) longdouble arrays: eta; l_ra, c_ra (response term and its condition); chi = (logT - mu)^2 / var; l, c (the whole cell)."""
        th, a, b = (np.asarray(v, dtype=LD) for v in (th, a, b))
        eta = a[None, :] * (th[:, None] - b[None, :])
        l_ra = -_log1pexp(-(2 * self.Y - 1) * eta)
        c_ra = np.abs(self.Y * eta) + np.abs(_log1pexp(eta))
        out = dict(eta=eta, l_ra=l_ra, c_ra=c_ra, l=l_ra, c=c_ra)
        if self.model != "mlirt":
            ze, lam, sg = (np.asarray(v, dtype=LD) for v in (ze, lam, sg))
            mu, var = lam[None, :] - ze[:, None], np.broadcast_to(sg[None, :], eta.shape)
            if self.model in ("cross", "crossqr"):
                mu = mu - th[:, None] * np.asarray(rho, dtype=LD)[None, :]
            if self.model == "crossqr":
                nu = np.asarray(nu, dtype=LD)
                mu, var = mu + self.k1 * nu, sg[None, :] * (self.k2 * nu)
            chi = (self.logT - mu) ** 2 / var
            l2pi = np.log(2 * LD(np.pi))
            out.update(chi=chi, l=l_ra - l2pi / 2 - np.log(var) / 2 - chi / 2, c=c_ra + l2pi / 2 + np.abs(np.log(var)) / 2 + chi / 2)
        return out

    def row(self, ra, rt, qr):
        """cells() at one trace row (Post.ra / rt / qr rows as parity_util.decode_rows reads them)."""
        N, J = self.N, self.J
        kw = {}
        if self.model != "mlirt":
            kw.update(ze=rt[:N], lam=rt[N:N + J], sg=rt[N + J:N + 2 * J])
        if self.model in ("cross", "crossqr"):
            kw["rho"] = qr[:J]
        if self.model == "crossqr":
            kw["nu"] = np.asarray(qr[J + 4:]).reshape(N, J, order="F")
        return self.cells(ra[:N], ra[N:N + J], ra[N + J:N + 2 * J], **kw)

    def loglik(self, P, X, F):
        """getLogLikelihood at a parameter point P (a dict with erm_get_mean's keys): (value, condition sum) with the subjects' structural terms included."""
        m, N = self.model, self.N
        th, ze = np.asarray(P["theta"], dtype=LD), None if m == "mlirt" else np.asarray(P["zeta"], dtype=LD)
        c = self.cells(th, P["a"], P["b"], ze, P.get("lambda_"), P.get("sig2t"), P.get("rho"), None if m != "crossqr" else np.asarray(P["nu"]).reshape(N, self.J, order="F"))
        ll, cond = c["l"].sum(), c["c"].sum()
        x = np.column_stack([np.ones(N)] + ([np.asarray(X, dtype=np.float64)] if F > 0 else [])).astype(LD)
        l2pi = np.log(2 * LD(np.pi))
        if m == "mlirt":
            e = th - x @ np.asarray(P["beta"], dtype=LD)
            return ll + (-l2pi / 2 - e * e / 2).sum(), cond + (l2pi / 2 + e * e / 2).sum()
        S = np.asarray(P["sigp"], dtype=LD).reshape(2, 2, order="F")
        if m in ("rtirt", "crossqr", "null", "cross"):
            e0, e1 = th, ze
            if m == "rtirt":
                xb = x @ np.asarray(P["beta"], dtype=LD).reshape(F + 1, 2, order="F")
                e0, e1 = th - xb[:, 0], ze - xb[:, 1]
            det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
            t = (S[1, 1] * e0 * e0, (S[0, 1] + S[1, 0]) * e0 * e1, S[0, 0] * e1 * e1)
            return ll + (-l2pi - np.log(det) / 2 - (t[0] - t[1] + t[2]) / det / 2).sum(), cond + (l2pi + np.abs(np.log(det)) / 2 + (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])) / np.abs(det) / 2).sum()
        nu = np.asarray(P["nu"], dtype=LD) if m == "latentqr" else LD(1)
        xx = np.column_stack([x, th])
        e, var = ze - (xx @ np.asarray(P["beta"], dtype=LD) + self.k1 * nu), S[1, 1] * self.k2 * nu
        return ll + (-l2pi / 2 - np.log(var) / 2 - e * e / var / 2).sum(), cond + (l2pi / 2 + np.abs(np.log(var)) / 2 + e * e / var / 2).sum()


def extended_reference(model, Y, logT, ra, rt, qr, *, n_iter, n_burnin, seed=1234, sweep0=1, qRt=0.85):
    """WAIC and the replicate pass of one chain (Post.ra / rt / qr in Julia layout, nChain = 1) in extended precision.  Returns a dict:
      L_subj, C_subj (n, N); L_cell, C_cell (n, N, J)                 l of every post-burn-in row and its condition sum
      ppc[unit][quantity] = (mean over the replicates of the value, of its condition sum), unit in subject / item / total,
                            quantity in D_obs, D_rep, DT_obs, DT_rep, T_rep (items only)."""
    G = pu.ge.load_package().twins
    N, J = Y.shape
    E = Extended(model, Y, logT, qRt)
    rows = range(n_burnin, n_iter)
    out = dict(L_subj=[], C_subj=[], L_cell=[], C_cell=[])
    acc = {u: collections.defaultdict(lambda: [LD(0), LD(0)]) for u in ("subject", "item", "total")}
    ii, jj = np.arange(N, dtype=np.uint64)[:, None], np.arange(J, dtype=np.uint64)[None, :]
    for it in rows:
        c = E.row(ra[it, :, 0], None if model == "mlirt" else rt[it, :, 0], qr[it, :, 0])
        out["L_subj"].append(c["l"].sum(axis=1)); out["C_subj"].append(c["c"].sum(axis=1)); out["L_cell"].append(c["l"]); out["C_cell"].append(c["c"])
        w0, w1, w2, _ = G._philox4x32_10(ii, jj, sweep0 + it, G._ppc_stream_word3(0), seed, seed >> 32)
        u0 = (w0.astype(LD) + LD(0.5)) * LD(2.0) ** -32
        yrep = (u0 < 1 / (1 + np.exp(-c["eta"]))).astype(LD)
        d = (E.Y - yrep) * c["eta"]
        q = {"D_obs": (-2 * c["l_ra"], 2 * c["c_ra"]), "D_rep": (-2 * c["l_ra"] + 2 * d, 2 * c["c_ra"] + 2 * np.abs(d)), "T_rep": (yrep, yrep)}
        if model != "mlirt":
            u1, u2 = (w1.astype(LD) + LD(0.5)) * LD(2.0) ** -32, (w2.astype(LD) + LD(0.5)) * LD(2.0) ** -32
            z2 = -2 * np.log(u1) * np.cos(2 * LD(np.pi) * u2) ** 2
            q.update(DT_obs=(c["chi"], c["chi"]), DT_rep=(z2, z2))
        for name, (v, cv) in q.items():
            for unit, ax in (("subject", 1), ("item", 0), ("total", None)):
                acc[unit][name][0] = acc[unit][name][0] + v.sum(axis=ax)
                acc[unit][name][1] = acc[unit][name][1] + cv.sum(axis=ax)
    n = len(rows)
    for k in ("L_subj", "C_subj", "L_cell", "C_cell"):
        out[k] = np.stack(out[k])
    out["ppc"] = {u: {name: (v[0] / n, v[1] / n) for name, v in a.items()} for u, a in acc.items()}
    out["n"] = n
    return out


def waic_bounds(L, C, c):
    """lppd_u, p_u of rows L (n, U) in extended precision and their bounds under `|l - ref| <= c 2^-53 cond`: lppd_u within the largest per-row bound delta_u (a
    log-mean-exp moves by at most the largest move of its arguments); p_u, the sample variance, within 2 sd_u delta' + delta'^2, delta' = delta_u sqrt(n / (n - 1)) --
    defined also where the reference variance is exactly zero.  The finish m + log(sum exp(l - m)) - log n adds roundings of its own that do not scale with l: n
    exponentials <= 1 and their sum (n 2^-53 relative to a sum >= 1), two logarithms and two additions -- (n + 4 + 2 log n) 2^-53 absolute on lppd_u, which is all
    that is left of a unit whose l is below 1e-15 in every row (an all-wrong subject at theta = -10; scipy's logsumexp, the twin's finish, has the same term).
    Returns (lppd_u, its bound, p_u, its bound)."""
    n = L.shape[0]
    m = L.max(axis=0)
    lppd = m + np.log(np.exp(L - m).sum(axis=0)) - np.log(LD(n))
    p = ((L - L.mean(axis=0)) ** 2).sum(axis=0) / (n - 1)
    delta = LD(c) * LD(U53) * C.max(axis=0) + LD(FLOOR)
    dp = delta * np.sqrt(LD(n) / (n - 1))
    finish = LD(n + 4 + 2 * np.log(n)) * LD(U53)
    # (p_u is an fp64 result of squares: below the smallest normal number -- deviations under 1e-154 -- it carries no relative precision either)
    return lppd, delta + finish, p, 2 * np.sqrt(p) * dp + dp * dp + LD(FLOOR)


def worst_ratio(got, ref, cond):
    """max (|got - ref| - FLOOR) / (2^-53 cond) over the entries (0 where the difference is within the floor)."""
    d = np.maximum(np.abs(np.asarray(got).astype(LD) - ref) - LD(FLOOR), 0)
    b = LD(U53) * np.asarray(cond, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / np.where(b > 0, b, 1), 0)
        r = np.where((d > 0) & ~(b > 0), np.inf, r)
    return float(np.max(r))


PPC_SLOTS = {"subject": {"D_obs": (0, 2), "D_rep": (0, 3), "DT_obs": (1, 2), "DT_rep": (1, 3)},
             "item": {"D_obs": (0, 2), "D_rep": (0, 3), "DT_obs": (1, 2), "DT_rep": (1, 3), "T_rep": (2, 3)},
             "total": {"D_obs": (0, 2), "D_rep": (0, 3), "DT_obs": (1, 2), "DT_rep": (1, 3)}}


def ppc_ratios(P, ref):
    """{(unit, quantity): worst_ratio} of an OutputPpc's means against extended_reference's."""
    arr = {"subject": P.subj, "item": P.item, "total": P.total}
    out = {}
    for unit, slots in PPC_SLOTS.items():
        for name, (comp, q) in slots.items():
            if name not in ref["ppc"][unit]:
                continue
            v, cv = ref["ppc"][unit][name]
            out[(unit, name)] = worst_ratio(arr[unit][comp, q], v, cv)
    return out


def assert_counts_equal_twin(dev, host, what=""):
    """ppc_util.assert_equals_twin's rule for the counts alone: equal for every unit the margin rule keeps, and the rule keeps all but MAX_EXCLUDED of the units."""
    assert dev.R == host.R
    ex = ppu.excluded_units(host)
    n_units = n_ex = 0
    for name, d, h in (("item", dev.item, host.item), ("subject", dev.subj, host.subj), ("total", dev.total, host.total)):
        for comp in range(d.shape[0]):
            if np.all(np.isnan(h[comp])):
                assert np.all(np.isnan(d[comp])), (name, comp)
                continue
            keep = ~np.atleast_1d(ex[name][comp])
            n_units += keep.size
            n_ex += int((~keep).sum())
            for q in (0, 1):
                assert np.array_equal(np.atleast_1d(d[comp, q])[keep], np.atleast_1d(h[comp, q])[keep]), (what, name, comp, q)
    print(f"{what}: counts equal, units excluded by the margin rule {n_ex} of {n_units}")
    assert n_ex <= ppu.MAX_EXCLUDED * n_units

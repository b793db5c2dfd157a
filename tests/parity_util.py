"""Test helpers: ctypes binding of the CPU oracle (oracle/liberm_oracle.so) and a runner that pushes the same seeded
inputs through the HIP library (via its C ABI) and through the oracle.  Test infrastructure only."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

MODELS = {"mlirt": 0, "rtirt": 1, "crossqr": 2, "latentqr": 3, "null": 4, "cross": 5, "latent": 6}
BASE = {"null": "rtirt", "cross": "crossqr", "latent": "latentqr"}      # data generator / layout family of each variant
_DP = C.POINTER(C.c_double)


class orc_config(C.Structure):
    _fields_ = [("model", C.c_int32), ("nItem", C.c_int32), ("nSubj", C.c_int64), ("nFeat", C.c_int32), ("intercept", C.c_int32),
                ("onepl", C.c_int32), ("cov2one", C.c_int32), ("chain", C.c_int32), ("sigp_mode", C.c_int32), ("qRt", C.c_double),
                ("seed", C.c_uint64)]


class orc_data(C.Structure):
    _fields_ = [("Y", C.c_void_p), ("logT", C.c_void_p), ("X", C.c_void_p)]


class orc_state(C.Structure):
    _fields_ = [(n, _DP) for n in ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "Sigp", "rho", "nu", "omega")]


_orc = None


def oracle():
    global _orc
    if _orc is None:
        ge.build_oracle()
        lib = C.CDLL(ge.ORACLE_LIB)
        lib.orc_run.argtypes = [C.POINTER(orc_config), C.POINTER(orc_data), C.POINTER(orc_state), C.c_int64, C.c_int64,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.orc_qr_width.argtypes = [C.POINTER(orc_config), C.c_int]
        lib.orc_loglik.argtypes = [C.POINTER(orc_config), C.POINTER(orc_data), C.POINTER(orc_state)]
        lib.orc_loglik.restype = C.c_double
        lib.orc_sample_batch.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.orc_sample_batch.restype = None
        lib.orc_philox.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.orc_philox.restype = None
        lib.orc_moments.argtypes = [C.POINTER(orc_config), C.POINTER(orc_data), C.POINTER(orc_state), C.c_int, C.c_void_p, C.c_void_p]
        lib.orc_moments.restype = None
        lib.orc_step.argtypes = [C.POINTER(orc_config), C.POINTER(orc_data), C.POINTER(orc_state), C.c_int, C.c_uint32]
        lib.orc_step.restype = None
        lib.orc_simulate_data.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 12
        lib.orc_simulate_data.restype = None
        lib.orc_set_threads.argtypes = [C.c_int]
        lib.orc_set_threads.restype = None
        _orc = lib
    return _orc


def orc_sample(which, n, par0=None, par1=None, *, seed=1234, site=15, sweep=1):
    out = np.empty(n, dtype=np.float64)
    p0 = None if par0 is None else np.ascontiguousarray(par0, dtype=np.float64)
    p1 = None if par1 is None else np.ascontiguousarray(par1, dtype=np.float64)
    oracle().orc_sample_batch(which, seed, site, sweep, n, None if p0 is None else p0.ctypes.data,
                              None if p1 is None else p1.ctypes.data, out.ctypes.data)
    return out


def orc_simulate(gen, N, J, F, *, a, b, lam=None, sig2t=None, rho=None, Sigp=None, beta=None, seed=4321, noise=0):
    """The oracle's restatement of setData* (gen 0 MlIrt, 1 RtIrt, 2 Null, 3 Cross, 4 Latent) with the device's stream addressing.
    Returns dict(X, theta, zeta, Y, logT), column-major."""
    def p(v):
        return None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, order="F"))
    a_, b_, l_, s_, r_, S_, B_ = p(a), p(b), p(lam), p(sig2t), p(rho), p(Sigp), p(beta)
    X = np.zeros((N, max(F, 1)), order="F")
    th, ze = np.zeros(N), np.zeros(N)
    Y = np.zeros((N, J), dtype=np.uint8, order="F")
    logT = np.zeros((N, J), order="F")
    ptr = lambda v: None if v is None else v.ctypes.data
    oracle().orc_simulate_data(gen, noise, seed, N, J, F, ptr(a_), ptr(b_), ptr(l_), ptr(s_), ptr(r_), ptr(S_), ptr(B_),
                               X.ctypes.data, th.ctypes.data, ze.ctypes.data, Y.ctypes.data, logT.ctypes.data)
    return dict(X=X[:, :F], theta=th, zeta=ze, Y=Y, logT=logT)


class OracleProblem:
    """Holds data + state arrays (column-major, fp64) in the oracle's structs."""

    def __init__(self, model, Y, logT, X, state, *, qRt=0.5, intercept=False, onepl=False, cov2one=True, seed=1234, chain=0, sigp_mode=0):
        self.model = MODELS[model] if isinstance(model, str) else model
        self.N, self.J = Y.shape
        self.F = 0 if X is None else X.shape[1]
        self.Y = np.asfortranarray(Y.astype(np.uint8))
        self.logT = None if logT is None else np.asfortranarray(logT, dtype=np.float64)
        self.X = None if X is None else np.asfortranarray(X, dtype=np.float64)
        self.cfg = orc_config(self.model, self.J, self.N, self.F, int(intercept), int(onepl), int(cov2one), chain, int(sigp_mode), qRt, seed)
        self.data = orc_data(self.Y.ctypes.data, None if self.logT is None else self.logT.ctypes.data,
                             None if self.X is None else self.X.ctypes.data)
        N, J, F = self.N, self.J, self.F
        nb = {0: F + 1, 1: 2 * (F + 1), 2: 1, 3: F + 2, 4: 2 * (F + 1), 5: 1, 6: F + 2}[self.model]
        nnu = {2: N * J, 3: N}.get(self.model, 1)
        self.arr = dict(theta=np.zeros(N), a=np.ones(J), b=np.zeros(J), zeta=np.zeros(N), lambda_=np.zeros(J), sig2t=np.ones(J),
                        beta=np.zeros(nb), Sigp=np.array([1.0, 0, 0, 1.0]), rho=np.zeros(J), nu=np.ones(nnu), omega=np.zeros(N * J))
        for k, v in state.items():
            k = {"lam": "lambda_", "sigp": "Sigp"}.get(k, k)
            if v is not None:
                self.arr[k][:] = np.asarray(v, dtype=np.float64).reshape(-1, order="F")
        self.st = orc_state(*[self.arr[n].ctypes.data_as(_DP) for n, _ in orc_state._fields_])
        self.sweeps = 0

    def qr_width(self, with_nu):
        return oracle().orc_qr_width(C.byref(self.cfg), int(with_nu))

    def run(self, nsweeps, with_nu=False):
        N, J = self.N, self.J
        ra = np.zeros((nsweeps, N + 2 * J))
        rt = np.zeros((nsweeps, N + 2 * J))
        qr = np.zeros((nsweeps, self.qr_width(with_nu)))
        ll = np.zeros(nsweeps)
        oracle().orc_run(C.byref(self.cfg), C.byref(self.data), C.byref(self.st), self.sweeps, nsweeps,
                         ra.ctypes.data, rt.ctypes.data, qr.ctypes.data, int(with_nu), ll.ctypes.data)
        self.sweeps += nsweeps
        return dict(ra=ra, rt=rt, qr=qr, ll=ll)

    def moments(self, which, n1, n2=1):
        o1, o2 = np.zeros(n1), np.zeros(max(n2, 1))
        oracle().orc_moments(C.byref(self.cfg), C.byref(self.data), C.byref(self.st), which, o1.ctypes.data, o2.ctypes.data)
        return o1, o2

    def step(self, step, t):
        oracle().orc_step(C.byref(self.cfg), C.byref(self.data), C.byref(self.st), step, t)

    def loglik(self):
        return oracle().orc_loglik(C.byref(self.cfg), C.byref(self.data), C.byref(self.st))


# ---------------------------------------------------------------------------------------------------------------
def make_problem(model, N, J, F=3, seed=7, qRt=0.85):
    """Synthetic inputs in the style of setData* (src/SimTools.jl) plus a constructor-style initial state."""
    pkg = ge.load_package()
    Cond = pkg.setCond(nSubj=N, nItem=J, nFeat=F, nIter=10, nChain=1, qRt=qRt)
    g = np.random.default_rng(seed)
    if model == "mlirt":
        tp = pkg.setTrueParaMlIrt(Cond, seed=g)
        D = pkg.setDataMlIrt(Cond, tp, seed=g)
        init = dict(theta=g.standard_normal(N), beta=g.standard_normal(F + 1))
        return D.Y, None, D.X, init, tp
    if model in ("rtirt", "null"):
        tp = pkg.setTrueParaRtIrt(Cond, seed=g)
        if model == "null":
            tp.beta = np.zeros((F, 2))          # the Null model has no covariate effects: theta, zeta ~ N(0, Sigp)
        D = pkg.setDataRtIrt(Cond, tp, seed=g)
        init = dict(theta=g.standard_normal(N), zeta=g.standard_normal(N), beta=g.standard_normal((F + 1, 2)), sigp=np.eye(2))
        if model == "null":
            init["beta"] = np.zeros((F + 1, 2))
        return D.Y, D.logT, D.X, init, tp
    if model in ("crossqr", "cross"):
        tp = pkg.setTrueParaRtIrtCross(Cond, seed=g)
        D = pkg.setDataRtIrtCross(Cond, tp, seed=g)
        init = dict(theta=g.standard_normal(N), zeta=g.standard_normal(N), rho=g.standard_normal(J), sigp=np.eye(2))
        return D.Y, D.logT, None, init, tp
    if model in ("latentqr", "latent"):
        tp = pkg.setTrueParaRtIrtLatent(Cond, seed=g)
        D = pkg.setDataRtIrtLatent(Cond, tp, seed=g)
        init = dict(theta=g.standard_normal(N), zeta=g.standard_normal(N), beta=g.standard_normal(F + 2), sigp=np.eye(2))
        return D.Y, D.logT, D.X, init, tp
    raise ValueError(model)


def run_device(model, Y, logT, X, init, nsweeps, *, precision="f64", qRt=0.85, seed=1234, intercept=False, onepl=False,
               cov2one=None, trace_full=True, n_chain=1, n_burnin=None, **opts):
    pkg = ge.load_package()
    L = pkg._lib
    N, J = Y.shape
    F = 0 if X is None else X.shape[1]
    if cov2one is None:
        cov2one = model not in ("latentqr", "latent")
    nb = nsweeps // 2 if n_burnin is None else n_burnin
    eng = L.Engine(model=MODELS[model], n_item=J, n_subj=N, n_feat=F, n_iter=nsweeps // n_chain, n_chain=n_chain, n_burnin=nb,
                   intercept=int(intercept), one_pl=int(onepl), cov2one=int(cov2one), q_rt=qRt, seed=seed,
                   precision={"f32": 0, "f64": 1}[precision], trace_mode=1 if trace_full else 0, **opts)
    eng.set_data(Y, logT, X)
    st = {("lambda_" if k == "lam" else k): v for k, v in init.items()}
    eng.set_state(**st)
    eng.run(nsweeps)
    out = dict(item=eng.item_trace(), ll=eng.trace(L.TRACE_LOGLIKE), state=eng.get_state(), engine=eng)
    if trace_full:
        out["ra"] = eng.trace(L.TRACE_RA)
        if model != "mlirt":
            out["rt"] = eng.trace(L.TRACE_RT)
        out["qr"] = eng.trace(L.TRACE_QR)
    return out


def run_pair(model, N, J, nsweeps, *, F=3, precision="f64", seed=7, qRt=0.85, **kw):
    """Same inputs through device and oracle.  Returns dict with device traces (rows x width) and oracle traces."""
    Y, logT, X, init, tp = make_problem(model, N, J, F, seed=seed, qRt=qRt)
    cov2one = kw.get("cov2one")
    if cov2one is None:
        cov2one = model not in ("latentqr", "latent")
    dev = run_device(model, Y, logT, X, init, nsweeps, precision=precision, qRt=qRt, **kw)
    op = OracleProblem(model, Y, logT, X, init, qRt=qRt, intercept=kw.get("intercept", False), onepl=kw.get("onepl", False),
                       cov2one=cov2one, seed=kw.get("seed", 1234), sigp_mode=kw.get("sigp_mode", 0))
    orc = op.run(nsweeps, with_nu=(model in ("latentqr", "crossqr")))
    d = dict(orc=orc, dev=dev, model=model)
    # device traces in Julia layout (nIter, width, nChain=1) -> rows x width
    d["dev_ra"] = dev["ra"][:, :, 0]
    if model != "mlirt":
        d["dev_rt"] = dev["rt"][:, :, 0]
    d["dev_qr"] = dev["qr"][:, :, 0]
    d["dev_ll"] = dev["ll"][:, 0, 0]
    return d


@contextlib.contextmanager
def oracle_threads(n):
    """The oracle's OpenMP mode for the enclosed runs (bit-identical to its single-thread run: tests/test_oracle_sweeps.py)."""
    oracle().orc_set_threads(int(n))
    try:
        yield
    finally:
        oracle().orc_set_threads(1)


def rel_err(x, y, floor=1e-6):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.abs(x - y) / np.maximum(np.abs(y), floor)


def max_rel_err(res, floor=1e-6):
    e = [rel_err(res["dev_ra"], res["orc"]["ra"], floor).max()]
    if res["model"] != "mlirt":
        e.append(rel_err(res["dev_rt"], res["orc"]["rt"], floor).max())
    e.append(rel_err(res["dev_qr"], res["orc"]["qr"], floor).max())
    e.append(rel_err(res["dev_ll"], res["orc"]["ll"], floor).max())
    return float(max(e))


def rel_err_by_part(res, floor=1e-6):
    """max_rel_err taken apart: {part: (largest error, sweep, column)} for the ra, rt, qr and ll traces of a run_pair result."""
    parts = [("ra", res["dev_ra"], res["orc"]["ra"])]
    if res["model"] != "mlirt":
        parts.append(("rt", res["dev_rt"], res["orc"]["rt"]))
    parts += [("qr", res["dev_qr"], res["orc"]["qr"]), ("ll", res["dev_ll"][:, None], np.asarray(res["orc"]["ll"])[:, None])]
    out = {}
    for name, d, o in parts:
        e = rel_err(d, o, floor)
        t, k = np.unravel_index(int(np.argmax(e)), e.shape)
        out[name] = (float(e[t, k]), int(t), int(k))
    return out


# ---------------------------------------------------------------------------------------------------------------
# The launch-geometry planner on the CPU: tests/geometry_check.cpp compiled against extendedrtirtmodeling.jl_amd/csrc/erm_geometry.hpp, the header
# Engine::init plans with.  `exe` is a pytest fixture (test modules import it by name); plan() runs the checker's `case` mode.
GEOMETRY_SRC = os.path.join(ROOT, "tests", "geometry_check.cpp")
GEOMETRY_INC = os.path.join(ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
ITEM_STRIDE = 128               # erm_layout.hpp: item_stride(J) is this constant for J <= 128 and J beyond
CQ_MODELS = ("crossqr", "cross")            # two row passes per sweep: never fused, never persistent


def build_geometry_check(out):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", GEOMETRY_INC, GEOMETRY_SRC, "-o", out], check=True)
    return out


try:
    import pytest
except ImportError:             # smoke() and bench.py use this module without pytest
    pytest = None
if pytest is not None:
    @pytest.fixture(scope="module")
    def exe(tmp_path_factory):
        return build_geometry_check(str(tmp_path_factory.mktemp("geom") / "geometry_check"))


def plan(exe, model, f64, N, J, Fk, bt=0, gb=0, W=0, cus=256, nofuse=0, nopersist=0, ngx=0):
    r = subprocess.run([exe, "case"] + [str(v) for v in (model, f64, N, J, Fk, bt, gb, W, cus, nofuse, nopersist, ngx)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip()
    if out.startswith("error="):
        return {"error": out[6:]}
    return dict(kv.split("=", 1) for kv in out.split())


def kernel_feat(model, F):
    """Covariate columns the kernels see (GeomIn.Fk): the Cross family and Null never read Data.X."""
    return 0 if model in CQ_MODELS or model == "null" else F


def extra_stats(model, F, sigp_mode=0):
    """GeomIn.ngx: GibbsRtIrtLatentQr with sigp_mode = 1 adds the 1/nu-weighted Gram statistics of [1 X theta | u], q = F + 2 columns: the packed upper
    triangle, the cross terms with u and the weight sum."""
    q = F + 2
    return q * (q + 1) // 2 + q + 1 if model == "latentqr" and sigp_mode == 1 else 0


def engine_plan(exe, model, precision, N, J, F, cu_count, *, lanes_per_row=0, block_threads=0, grid_blocks=0, flags=0, sigp_mode=0, refusal=False):
    """The CPU planner's plan for an engine's (model, precision, N, J, F, overrides, schedule flags) on a card with `cu_count` compute units, as integers;
    with `refusal`, a shape the planner turns down comes back as {"error": its message}."""
    p = plan(exe, MODELS[model], int(precision == "f64"), N, J, kernel_feat(model, F), bt=block_threads, gb=grid_blocks, W=lanes_per_row, cus=cu_count,
             nofuse=int(bool(flags & 1)), nopersist=int(bool(flags & 8)),          # ERM_FLAG_NO_FUSE = 1, ERM_FLAG_NO_PERSIST = 8 (include/ertirt.h)
             ngx=extra_stats(model, F, sigp_mode))
    if refusal and "error" in p:
        return p
    assert "error" not in p, p
    return {k: int(v) for k, v in p.items()}


def assert_engine_runs_plan(tm, p):
    """erm_get_timing of an engine against the CPU planner's plan for the same inputs: the launch geometry, the LDS request and the schedule."""
    got = (tm["lanes_per_row"], tm["block_threads"], tm["grid_blocks"], tm["lds_bytes"], tm["persistent"])
    want = (p["W"], p["block_threads"], p["grid_blocks"], max(p["lds0"], p["lds1"]), p["persist"])
    assert got == want, f"engine runs (W, threads, grid, lds, persistent) = {got}, the planner says {want}"
    assert tm["persist_fallbacks"] == 0, tm


# ---------------------------------------------------------------------------------------------------------------
# Adversarial data sets: the regions real data reaches and make_problem's defaults do not (separated items, saturated states, degenerate
# response patterns, raw log-millisecond times, covariates with a large offset).  Every one is a valid input to erm_set_data / erm_set_state.
EXTREME_KINDS = ("separated", "saturated", "degenerate", "rt_offset", "x_offset")
X_MODELS = ("mlirt", "rtirt", "latentqr", "latent")         # the models whose sampler reads Data.X


def extreme_models(kind):
    """The models a kind applies to: rt_offset needs response times, x_offset covariates."""
    if kind == "rt_offset":
        return [m for m in MODELS if m != "mlirt"]
    if kind == "x_offset":
        return list(X_MODELS)
    return list(MODELS)


def _simulate_y(g, theta, a, b):
    eta = a[None, :] * (theta[:, None] - b[None, :])
    return (g.random(eta.shape) < 0.5 * (1.0 + np.tanh(0.5 * eta))).astype(np.uint8)


def make_extreme_problem(kind, model, N, J, F=3, seed=11):
    """make_problem's data set and initial state, pushed into one edge region of the kernels.  Returns (Y, logT, X, init, truth) like
    make_problem; `init` always holds theta, a and b, so the first sweep's Polya-Gamma arguments z = |a_j (theta_i - b_j)| / 2 are fixed
    by the generator (pg_cell_coverage).
      separated   a log-uniform on [2, 8], theta with sd 3 and four subjects at +-10, Y simulated from them; init near the truth
      saturated   separated, then an injected state: items with a = 100 and 50, subjects at theta = +-20 (|eta| up to ~2 000)
      degenerate  all-1 and all-0 items, all-1 and all-0 subjects, one item with a single correct response
      rt_offset   logT in raw log-milliseconds (lambda ~ 8), one item with sigma2_t ~ 1e-4, one constant logT column, zeta offset by +3
      x_offset    X = [uniform on [20, 70], 0/1 dummy with 5 % ones, N(0, 1)]"""
    if kind not in EXTREME_KINDS:
        raise ValueError(kind)
    if model not in extreme_models(kind):
        raise ValueError(f"{kind} does not apply to {model}")
    Y, logT, X, init, tp = make_problem(model, N, J, F, seed=seed)
    g = np.random.default_rng(seed + 1000 * (EXTREME_KINDS.index(kind) + 1))
    init = dict(init)
    init.setdefault("a", np.ones(J))
    init.setdefault("b", np.zeros(J))
    Y = np.asfortranarray(Y.copy())
    if kind in ("separated", "saturated"):
        a = np.exp(g.uniform(np.log(2.0), np.log(8.0), J))
        b = g.normal(0.0, 0.5, J)
        theta = g.normal(0.0, 3.0, N)
        theta[:4] = (10.0, -10.0, 10.0, -10.0)
        Y = np.asfortranarray(_simulate_y(g, theta, a, b))
        tp.a, tp.b, tp.theta = a, b, theta
        init["theta"] = theta + 0.05 * g.standard_normal(N)
        init["a"] = a * np.exp(0.02 * g.standard_normal(J))
        init["b"] = b + 0.02 * g.standard_normal(J)
        if kind == "saturated":
            init["a"][:2] = (100.0, 50.0)
            init["theta"][:4] = (20.0, -20.0, 20.0, -20.0)
    elif kind == "degenerate":
        Y[0:3, :] = 1                      # all-correct subjects
        Y[3:6, :] = 0                      # all-wrong subjects (apart from the all-1 items below: the items are exact)
        Y[:, 0:2] = 1                      # items every subject answers correctly
        Y[:, 2:4] = 0                      # items every subject answers wrongly
        Y[:, 4] = 0
        Y[N // 2, 4] = 1                   # an item answered correctly by exactly one subject
    elif kind == "rt_offset":
        # raw log-milliseconds: every logT shifted to lambda ~ 8; the initial state is the truth with zeta offset by +3 and lambda by the
        # same +3 (the chain starts consistent with the data, so item 0 keeps its tiny residual variance instead of drifting towards it)
        lam = np.asarray(tp.lam, dtype=np.float64)
        shift = 8.0 - lam.mean()
        logT = np.asfortranarray(logT + shift)
        theta, zeta = np.asarray(tp.theta, dtype=np.float64), np.asarray(tp.zeta, dtype=np.float64)
        mu = lam[0] + shift - zeta               # (Cross family: rho_0 = 0, so item 0's residual does not move with each sweep's theta)
        logT[:, 0] = mu + 1e-2 * g.standard_normal(N)       # within-item residual variance ~1e-4
        logT[:, 1] = 8.0                                    # a constant column
        init["theta"] = theta + 1e-3 * g.standard_normal(N)
        init["zeta"] = zeta + 3.0 + 1e-3 * g.standard_normal(N)
        init["lam"] = lam + shift + 3.0
        sig2t = np.array(getattr(tp, "sig2t", None) if np.size(getattr(tp, "sig2t", None)) == J else np.ones(J), dtype=np.float64)
        sig2t[0] = 1e-4
        init["sig2t"] = sig2t
        if model in ("crossqr", "cross"):
            init["rho"] = np.array(tp.rho, dtype=np.float64)
            init["rho"][0] = 0.0
    elif kind == "x_offset":
        X = np.asfortranarray(np.column_stack([g.uniform(20.0, 70.0, N), (g.random(N) < 0.05).astype(np.float64), g.standard_normal(N)]))
        if X.shape[1] != F:
            X = np.asfortranarray(X[:, :F]) if F < 3 else np.asfortranarray(np.column_stack([X, g.standard_normal((N, F - 3))]))
    return Y, logT, X, init, tp


PG_BIN_WIDTH = 1.0 / 16.0       # the proposal table's z-bins (erm_rng.hpp pg_bin: bin k covers [k/16, (k+1)/16), 128 bins below z = 8)


def pg_cell_coverage(theta, a, b):
    """Where a state puts the cells' Polya-Gamma arguments z = |a_j (theta_i - b_j)| / 2: the histogram over the 128 proposal bins (z < 8),
    the fraction of cells with z >= 8 (the reference form), the counts with z >= 48 (p underflows in the mixture weight) and z > 745 (so
    does 2 e^{-z}), and the largest z."""
    theta, a, b = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (theta, a, b))
    z = 0.5 * np.abs(a[None, :] * (theta[:, None] - b[None, :]))
    lo = z[z < 8.0]
    hist = np.bincount(np.minimum((lo / PG_BIN_WIDTH).astype(np.int64), 127), minlength=128)
    return dict(hist=hist, bins_hit=int(np.count_nonzero(hist)), frac_ge8=float(np.mean(z >= 8.0)), n_ge48=int(np.sum(z >= 48.0)),
                n_gt745=int(np.sum(z > 745.0)), zmax=float(z.max()), eta_max=float(2.0 * z.max()))


# ---------------------------------------------------------------------------------------------------------------
_TF_NAMES = dict(theta="theta", a="a", b="b", zeta="zeta", lambda_="lambda_", sig2t="sig2t", beta="beta", sigp="Sigp", rho="rho", nu="nu")


_MLIRT_UNUSED = ("zeta", "lambda_", "sig2t", "sigp", "rho")


def _install_oracle_state(op, model, dev):
    """The device's state (erm_get_state: everything the next sweep reads, nu included) as the oracle's state."""
    for k, v in _TF_NAMES.items():
        if dev.get(k) is None or (model == "mlirt" and k in _MLIRT_UNUSED) or (k == "nu" and model not in ("crossqr", "latentqr")):
            continue
        op.arr[v][:] = dev[k]


def teacher_forced(model, Y, logT, X, init, T, precision, check, *, chunk=1, qRt=0.85, cov2one=None, seed=1234, **engine_opts):
    """Teacher forcing: every sweep of the device is compared with ONE oracle sweep from the state that sweep started from, so each
    conditional is checked on realistic chain states without error accumulation.  T sweeps in blocks of `chunk`; each block starts
    from the oracle's state (erm_set_state: the prologue's row pass draws omega), and its later sweeps are erm_runs that CONTINUE the chain
    -- they consume the Polya-Gamma draws the sweep kernel itself made (persistent or per-sweep), not the prologue's -- and are compared with
    an oracle sweep from the device's own state after the sweep before.  After
    each run check(t, dev_state, oracle_arrays) is called with t the index of the run's first sweep.
    Returns dict(engine, dev=(ra, rt, qr, ll) traces as rows x width, orc=the matching oracle rows)."""
    L = ge.load_package()._lib
    if cov2one is None:
        cov2one = model not in ("latentqr", "latent")
    op = OracleProblem(model, Y, logT, X, init, qRt=qRt, cov2one=cov2one, seed=seed)
    eng = L.Engine(model=MODELS[model], n_item=Y.shape[1], n_subj=Y.shape[0], n_feat=0 if X is None else X.shape[1], n_iter=T, n_chain=1,
                   n_burnin=0, cov2one=int(cov2one), q_rt=qRt, seed=seed, precision={"f32": 0, "f64": 1}[precision], trace_mode=1, **engine_opts)
    eng.set_data(Y, logT, X)
    orc = []
    for t in range(0, T, chunk):
        n = min(chunk, T - t)
        st = {k: op.arr[v].copy() for k, v in _TF_NAMES.items()}
        if model not in ("crossqr", "latentqr"):
            st.pop("nu")
        if model == "crossqr" and t == 0:
            st.pop("nu")           # constructors leave nu unset; it is drawn first
        eng.set_state(**st)
        for s_ in range(n):
            if s_ > 0:
                _install_oracle_state(op, model, dev)      # the run continues: the oracle takes the device's state after its previous sweep
            eng.run(1)                                      # (a continuing erm_run skips the prologue: its omega is the sweep kernel's own draw)
            orc.append(op.run(1, with_nu=model in ("crossqr", "latentqr")))
            dev = eng.get_state()
        check(t, {k: (None if dev[k] is None or (model == "mlirt" and k in _MLIRT_UNUSED) else dev[k]) for k in _TF_NAMES},
              {k: op.arr[v] for k, v in _TF_NAMES.items()})
    out = dict(engine=eng, orc={k: np.concatenate([o[k] for o in orc]) for k in ("ra", "rt", "qr", "ll")})
    out["dev"] = dict(ra=eng.trace(L.TRACE_RA)[:, :, 0], ll=eng.trace(L.TRACE_LOGLIKE)[:, 0, 0], qr=eng.trace(L.TRACE_QR)[:, :, 0])
    if model != "mlirt":
        out["dev"]["rt"] = eng.trace(L.TRACE_RT)[:, :, 0]
    return out


# ---------------------------------------------------------------------------------------------------------------
# Post.mean from the traces.  The column layouts are restated here from the interface (include/ertirt.h: erm_state, erm_get_trace) and the
# reference's Post.ra / rt / qr rows; nothing is imported from the code under test.
NU_MODELS = ("crossqr", "latentqr")
U53 = 2.0 ** -53                 # unit round-off of fp64


def trace_rows(tr):
    """A trace in Julia layout (nIter, width, nChain) as rows x width in the order the sweeps ran: sweep (m, l) is row m * nChain + l."""
    tr = np.asarray(tr)
    if tr.ndim == 2:
        return tr
    return np.ascontiguousarray(tr.transpose(0, 2, 1).reshape(tr.shape[0] * tr.shape[2], tr.shape[1]))


def decode_rows(model, N, J, F, ra, rt, qr):
    """Trace rows (rows x width) -> the fields of erm_state, each rows x size:
      ra = [theta (N); a (J); b (J)], rt = [zeta (N); lambda (J); sig2t (J)] (MlIrt has no rt: pass None),
      qr: MlIrt beta (F+1); RtIrt vec(beta) (2(F+1)), vec(Sigp) (4); Null the same with beta = 0; Cross rho (J), vec(Sigp);
          CrossQr rho, vec(Sigp), vec(nu) (N*J, column-major); Latent beta (F+2), vec(Sigp); LatentQr beta (F+2), vec(Sigp), nu (N).
    A quantile model's qr without its nu block (width J+4 / F+6) decodes without `nu`."""
    ra, qr = np.atleast_2d(np.asarray(ra, dtype=np.float64)), np.atleast_2d(np.asarray(qr, dtype=np.float64))
    if ra.shape[1] != N + 2 * J:
        raise ValueError(f"ra has {ra.shape[1]} columns, expected {N + 2 * J}")
    f = dict(theta=ra[:, :N], a=ra[:, N:N + J], b=ra[:, N + J:])
    if model != "mlirt":
        rt = np.atleast_2d(np.asarray(rt, dtype=np.float64))
        if rt.shape != ra.shape:
            raise ValueError(f"rt is {rt.shape}, expected {ra.shape}")
        f.update(zeta=rt[:, :N], lambda_=rt[:, N:N + J], sig2t=rt[:, N + J:])
    nb = {"mlirt": F + 1, "rtirt": 2 * (F + 1), "null": 2 * (F + 1), "cross": 0, "crossqr": 0, "latent": F + 2, "latentqr": F + 2}[model]
    nnu = {"crossqr": N * J, "latentqr": N}.get(model, 0)
    base = nb + (J if model in ("cross", "crossqr") else 0) + (0 if model == "mlirt" else 4)
    if qr.shape[0] != ra.shape[0] or qr.shape[1] not in (base, base + nnu):
        raise ValueError(f"qr is {qr.shape}, expected {ra.shape[0]} x {base}" + (f" or {base + nnu}" if nnu else ""))
    o = 0
    if model in ("cross", "crossqr"):
        f["rho"] = qr[:, :J]
        o = J
    elif model == "null":
        f["beta"] = np.zeros((qr.shape[0], nb))
        o = nb
    else:
        f["beta"] = qr[:, :nb]
        o = nb
    if model != "mlirt":
        f["sigp"] = qr[:, o:o + 4]
        o += 4
    if nnu and qr.shape[1] == base + nnu:
        f["nu"] = qr[:, o:]
    return f


def expected_mean(fields, n_burnin, n_chain):
    """Post.mean of decoded trace rows: the reference's joint mean over iterations m > nBurnin and all chains, i.e. over rows
    r >= n_burnin * n_chain.  Summed and divided in np.longdouble (64-bit significand: adding a few thousand fp64 values loses
    less than 2^-11 of one fp64 round-off), so the reference side carries no summation error an fp64 bound would see.
    Returns (mean, abs_sum, n): dicts of longdouble vectors -- the mean and sum |x_t| over the same rows -- and the row count."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("np.longdouble is not wider than fp64 on this platform")
    lo = int(n_burnin) * int(n_chain)
    mean, asum, n = {}, {}, 0
    for k, v in fields.items():
        x = np.asarray(v)[lo:].astype(np.longdouble)
        n = x.shape[0]
        if n <= 0:
            raise ValueError("no post-burn-in rows")
        mean[k] = x.sum(axis=0) / np.longdouble(n)
        asum[k] = np.abs(x).sum(axis=0)
    return mean, asum, n


def mean_excess(dev, mean, abs_sum, n, extra=2):
    """How far a device mean is outside its rounding bound, in units of the bound (<= 1 passes).  The device adds n post-burn-in draws in
    fp64 in row order (error <= (n - 1) u sum|x_t|) and multiplies by the rounded 1 / n (two more roundings):
    |dev - ref| <= (n + extra) u sum|x_t| / n, entry by entry.  An entry whose draws are all zero must be exactly zero."""
    d = np.abs(np.asarray(dev).astype(np.longdouble) - mean)
    bound = np.longdouble(n + extra) * np.longdouble(U53) * abs_sum / np.longdouble(n)
    out = np.zeros(d.shape, dtype=np.float64)
    nz = bound > 0
    out[nz] = (d[nz] / bound[nz]).astype(np.float64)
    out[~nz & (d > 0)] = np.inf
    return out

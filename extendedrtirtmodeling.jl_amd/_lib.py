"""ctypes binding of libertirt.so (include/ertirt.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from types import MappingProxyType

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ERM_LIB_PATH") or os.path.join(_HERE, "libertirt.so")      # ERM_LIB_PATH: diagnostics (library build variants)

MODEL_MLIRT, MODEL_RTIRT, MODEL_CROSSQR, MODEL_LATENTQR = 0, 1, 2, 3
MODEL_NULL, MODEL_CROSS, MODEL_LATENT = 4, 5, 6          # the non-quantile variants
PREC_F32, PREC_F64 = 0, 1
TRACE_SUMMARY, TRACE_FULL = 0, 1
TRACE_RA, TRACE_RT, TRACE_QR, TRACE_LOGLIKE = 0, 1, 2, 3

# What distinguishes the models on the host -- the same table as csrc/erm_model.hpp (model_traits), entry for entry (tests/test_model_traits.py):
#   rt: response times (logT, zeta, lambda, sig2t, Sigp, Post.rt);  rho: the cross-relation;  nu: "none" | "subject" (N) | "cell" (N x J);
#   sees_x: the kernels read Data.X;  beta: "none" | "vec" (nFeat+1) | "pair" ((nFeat+1) x 2) | "latent" (nFeat+2) | "zero_pair" (Null: a pair that is
#   always zero);  gen: the erm_simulate_data generator (0 MlIrt, 1 RtIrt, 2 Null, 3 Cross, 4 Latent)
ModelTraits = namedtuple("ModelTraits", "rt rho nu sees_x beta gen")
MODEL_TRAITS = MappingProxyType({
    MODEL_MLIRT: ModelTraits(False, False, "none", True, "vec", 0),
    MODEL_RTIRT: ModelTraits(True, False, "none", True, "pair", 1),
    MODEL_CROSSQR: ModelTraits(True, True, "cell", False, "none", 3),
    MODEL_LATENTQR: ModelTraits(True, False, "subject", True, "latent", 4),
    MODEL_NULL: ModelTraits(True, False, "none", False, "zero_pair", 2),
    MODEL_CROSS: ModelTraits(True, True, "none", False, "none", 3),
    MODEL_LATENT: ModelTraits(True, False, "none", True, "latent", 4),
})


def beta_shape(model, F):
    """Para.beta's shape: () when the model has none (or, for Null, never draws one)."""
    return {"none": (), "vec": (F + 1,), "pair": (F + 1, 2), "latent": (F + 2,), "zero_pair": (F + 1, 2)}[MODEL_TRAITS[model].beta]


def nbeta(model, F):
    """Entries of erm_state.beta (Null's are reported as zeros): beta_len of csrc/erm_model.hpp."""
    return {"none": 0, "vec": F + 1, "pair": 2 * (F + 1), "latent": F + 2, "zero_pair": 2 * (F + 1)}[MODEL_TRAITS[model].beta]


def nu_len(model, N, J):
    return {"none": 0, "subject": N, "cell": N * J}[MODEL_TRAITS[model].nu]


def kernel_feat(model, F):
    """Covariate columns the kernels see: the Cross family and Null never touch Data.X."""
    return F if MODEL_TRAITS[model].sees_x else 0

EXPORTS = [
    "erm_create", "erm_destroy", "erm_set_data", "erm_set_state", "erm_get_state", "erm_run", "erm_rows_done",
    "erm_reset_trace", "erm_trace_width", "erm_get_trace", "erm_item_trace_width", "erm_get_item_trace", "erm_get_mean",
    "erm_post_count", "erm_get_diagnostics", "erm_simulate_data", "erm_get_truth", "erm_get_data", "erm_get_timing", "erm_last_error", "erm_version", "erm_debug_sample", "erm_sample_gig",
    "erm_set_shard", "erm_copy", "erm_rccl_unique_id", "erm_set_shard_rccl",
    "erm_farm_create", "erm_farm_destroy", "erm_farm_chains", "erm_farm_engine", "erm_farm_set_data", "erm_farm_set_state", "erm_farm_get_state",
    "erm_farm_run", "erm_farm_reset_trace", "erm_farm_get_trace", "erm_farm_get_mean", "erm_farm_post_count", "erm_farm_used_rccl", "erm_farm_get_timing",
    "erm_get_dic", "erm_set_seed", "erm_farm_get_dic", "erm_farm_set_seed", "erm_abi_version", "erm_debug_invwishart", "erm_get_convergence", "erm_debug_convergence",
    "erm_set_pointwise", "erm_get_waic", "erm_pointwise_units", "erm_get_pointwise",
    "erm_set_predictive", "erm_predictive_reps", "erm_get_predictive",
    "erm_get_rank_diagnostics", "erm_get_rank_convergence", "erm_debug_rank_diagnostics",
    "erm_farm_get_diagnostics", "erm_farm_get_convergence", "erm_farm_get_rank_diagnostics", "erm_farm_get_rank_convergence", "erm_debug_diagnostics",
    "erm_get_marginal_waic", "erm_farm_get_marginal_waic", "erm_marginal_loglik",
    "erm_get_scores", "erm_farm_get_scores", "erm_score",
    "erm_get_marginal_loo", "erm_farm_get_marginal_loo", "erm_psis_loo",
    "erm_get_plausible_values", "erm_farm_get_plausible_values", "erm_plausible_values",
    "erm_get_quantile_marginal_waic", "erm_farm_get_quantile_marginal_waic", "erm_get_quantile_marginal_loo", "erm_farm_get_quantile_marginal_loo",
    "erm_quantile_marginal_loglik",
    "erm_marginal_loglik_masked", "erm_score_masked", "erm_plausible_values_masked",
    "erm_get_person_fit", "erm_farm_get_person_fit", "erm_person_fit", "erm_person_fit_masked",
    "erm_get_item_fit", "erm_farm_get_item_fit", "erm_item_fit",
]
ABI_VERSION = 4            # ERM_ABI_VERSION of the include/ertirt.h these ctypes structs mirror


class ErmError(RuntimeError):
    pass


class erm_config(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("n_item", C.c_int32), ("n_subj", C.c_int64), ("n_feat", C.c_int32), ("n_iter", C.c_int32),
        ("n_chain", C.c_int32), ("n_burnin", C.c_int32), ("intercept", C.c_int32), ("one_pl", C.c_int32),
        ("cov2one", C.c_int32), ("sigp_mode", C.c_int32), ("chain_id", C.c_int32), ("q_rt", C.c_double),
        ("seed", C.c_uint64), ("device", C.c_int32), ("precision", C.c_int32), ("trace_mode", C.c_int32),
        ("lanes_per_row", C.c_int32), ("block_threads", C.c_int32), ("grid_blocks", C.c_int32), ("profile", C.c_int32),
        ("flags", C.c_int32), ("nu_trace_max_gb", C.c_double),
    ]


POINTWISE_OFF, POINTWISE_SUBJECT, POINTWISE_CELL = 0, 1, 2      # erm_set_pointwise: the unit of WAIC
POINTWISE_UNITS = {None: POINTWISE_OFF, "subject": POINTWISE_SUBJECT, "cell": POINTWISE_CELL}
FLAG_NO_FUSE, FLAG_NO_GRAPH, FLAG_FARM_FORCE_RCCL, FLAG_NO_PERSIST, FLAG_TEST_PERSIST_TIMEOUT = 1, 2, 4, 8, 16


class erm_farm_timing(C.Structure):
    _fields_ = [("run_wall_ms", C.c_double), ("gather_ms", C.c_double), ("allreduce_ms", C.c_double), ("comm_init_ms", C.c_double), ("rccl_ranks", C.c_int32), ("n_devices", C.c_int32)]


_DP = C.POINTER(C.c_double)


class erm_state(C.Structure):
    _fields_ = [(n, _DP) for n in ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp", "rho", "nu")]


class erm_timing(C.Structure):
    _fields_ = [
        ("run_ms", C.c_double), ("pass_ms_total", C.c_double), ("event_overhead_ms", C.c_double), ("pass_launches", C.c_int64), ("sweeps", C.c_int64),
        ("lanes_per_row", C.c_int32), ("block_threads", C.c_int32), ("grid_blocks", C.c_int32), ("lds_bytes", C.c_int32),
        ("cu_count", C.c_int32), ("persistent", C.c_int32), ("persist_fallbacks", C.c_int32), ("reserved_", C.c_int32),
    ]


# int (*erm_exchange_fn)(void* user, const void* dev_send, void* dev_recv, size_t bytes_per_rank)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)

_lib = None


def load():
    """Load libertirt.so; raises ErmError if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ErmError(f"HIP extension missing: {LIB_PATH} (build it with `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(LIB_PATH)
    lib.erm_abi_version.restype = C.c_int
    if lib.erm_abi_version() != ABI_VERSION:
        raise ErmError(f"{LIB_PATH} has struct layout version {lib.erm_abi_version()}, this binding was written against {ABI_VERSION}: rebuild the library")
    H = C.c_void_p
    lib.erm_create.argtypes = [C.POINTER(erm_config), C.POINTER(H)]
    lib.erm_destroy.argtypes = [H]
    lib.erm_destroy.restype = None
    lib.erm_set_data.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_set_state.argtypes = [H, C.POINTER(erm_state)]
    lib.erm_get_state.argtypes = [H, C.POINTER(erm_state)]
    lib.erm_run.argtypes = [H, C.c_int64]
    lib.erm_rows_done.argtypes = [H]
    lib.erm_rows_done.restype = C.c_int64
    lib.erm_reset_trace.argtypes = [H]
    lib.erm_trace_width.argtypes = [H, C.c_int]
    lib.erm_trace_width.restype = C.c_int64
    lib.erm_get_trace.argtypes = [H, C.c_int, C.c_void_p]
    lib.erm_item_trace_width.argtypes = [H]
    lib.erm_item_trace_width.restype = C.c_int64
    lib.erm_get_item_trace.argtypes = [H, C.c_void_p]
    lib.erm_get_mean.argtypes = [H, C.POINTER(erm_state)]
    lib.erm_post_count.argtypes = [H]
    lib.erm_post_count.restype = C.c_int64
    lib.erm_simulate_data.argtypes = [H, C.POINTER(erm_state), C.c_uint64, C.c_int]
    lib.erm_get_truth.argtypes = [H, C.c_void_p, C.c_void_p]
    lib.erm_get_data.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_get_timing.argtypes = [H, C.POINTER(erm_timing)]
    lib.erm_last_error.restype = C.c_char_p
    lib.erm_version.restype = C.c_char_p
    lib.erm_debug_sample.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_sample_gig.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.erm_set_shard.argtypes = [H, C.c_int, C.c_int, C.c_int64, C.c_int64, EXCHANGE_FN, C.c_void_p]
    lib.erm_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.erm_rccl_unique_id.argtypes = [C.c_void_p]
    lib.erm_set_shard_rccl.argtypes = [H, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    lib.erm_farm_create.argtypes = [C.POINTER(erm_config), C.POINTER(C.c_int32), C.c_int32, C.POINTER(H)]
    lib.erm_farm_destroy.argtypes = [H]
    lib.erm_farm_destroy.restype = None
    lib.erm_farm_chains.argtypes = [H]
    lib.erm_farm_chains.restype = C.c_int32
    lib.erm_farm_engine.argtypes = [H, C.c_int32]
    lib.erm_farm_engine.restype = H
    lib.erm_farm_set_data.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_farm_set_state.argtypes = [H, C.c_int32, C.POINTER(erm_state)]
    lib.erm_farm_get_state.argtypes = [H, C.c_int32, C.POINTER(erm_state)]
    lib.erm_farm_run.argtypes = [H, C.c_int64]
    lib.erm_farm_reset_trace.argtypes = [H]
    lib.erm_farm_get_trace.argtypes = [H, C.c_int, C.c_void_p]
    lib.erm_farm_get_mean.argtypes = [H, C.POINTER(erm_state)]
    lib.erm_farm_post_count.argtypes = [H]
    lib.erm_farm_post_count.restype = C.c_int64
    lib.erm_farm_used_rccl.argtypes = [H]
    lib.erm_farm_get_timing.argtypes = [H, C.POINTER(erm_farm_timing), C.c_void_p]
    lib.erm_get_dic.argtypes = [H, C.c_void_p]
    lib.erm_debug_convergence.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_set_pointwise.argtypes = [H, C.c_int]
    lib.erm_get_waic.argtypes = [H, C.c_void_p]
    lib.erm_pointwise_units.argtypes = [H]
    lib.erm_pointwise_units.restype = C.c_int64
    lib.erm_get_pointwise.argtypes = [H, C.c_void_p, C.c_void_p]
    lib.erm_set_predictive.argtypes = [H, C.c_int, C.c_int32]
    lib.erm_predictive_reps.argtypes = [H]
    lib.erm_predictive_reps.restype = C.c_int64
    lib.erm_get_predictive.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_set_seed.argtypes = [H, C.c_uint64]
    lib.erm_farm_get_dic.argtypes = [H, C.c_void_p]
    lib.erm_farm_set_seed.argtypes = [H, C.c_uint64]
    lib.erm_debug_invwishart.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
    lib.erm_debug_rank_diagnostics.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.erm_debug_diagnostics.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    I32, VP = C.c_int32, C.c_void_p
    stems = [fam.stem for fam in MARGINAL_FAMILIES.values()]
    pairs = [("diagnostics", [C.c_int, VP, VP]), ("convergence", [C.c_int, VP]), ("rank_diagnostics", [C.c_int, VP, VP, VP]), ("rank_convergence", [C.c_int, VP]),
             ("scores", [I32, VP, VP]), ("person_fit", [I32, VP, VP]), ("item_fit", [I32, VP, VP]), ("plausible_values", [I32, I32, C.c_uint64, VP, VP, VP, VP])]
    pairs += [(stem + "waic", [I32, VP, VP, VP]) for stem in stems] + [(stem + "loo", [I32, VP, VP]) for stem in stems]
    for prefix in ("erm_get_", "erm_farm_get_"):          # every pair that _Diagnostics and _ItemPasses resolve through _get_prefix
        for name, args in pairs:
            getattr(lib, prefix + name).argtypes = [H] + args
    head = [C.c_int, C.c_int, C.c_int64, I32, I32, VP, VP, VP, VP, C.c_int64]      # the caller-data entries: device, model, N, J, F, Y, logT, X, rows, R (_caller_head)
    for fam in MARGINAL_FAMILIES.values():
        getattr(lib, fam.loglik).argtypes = head + [C.c_double] * len(fam.scalars) + [I32, VP, VP, VP, VP]
    lib.erm_score.argtypes = head + [I32, I32, VP, VP]
    lib.erm_psis_loo.argtypes = [C.c_int, VP, C.c_int64, C.c_int64, VP, VP, VP]
    lib.erm_plausible_values.argtypes = head + [I32, I32, C.c_uint64, VP, VP, VP, VP]
    mhead = head[:8] + [VP] + head[8:]      # the masked entries: obs between X and rows, n_obs last
    lib.erm_marginal_loglik_masked.argtypes = mhead + [I32, VP, VP, VP, VP, VP]
    lib.erm_score_masked.argtypes = mhead + [I32, I32, VP, VP, VP]
    lib.erm_plausible_values_masked.argtypes = mhead + [I32, I32, C.c_uint64, VP, VP, VP, VP, VP]
    lib.erm_person_fit.argtypes = head + [I32, I32, VP, VP]
    lib.erm_person_fit_masked.argtypes = mhead + [I32, I32, VP, VP, VP]
    lib.erm_item_fit.argtypes = mhead + [I32, VP, VP]      # (obs may be NULL; no weighting, no n_obs)
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise ErmError(f"libertirt error {rc}: {load().erm_last_error().decode()}")


MARGINAL_MODELS = (MODEL_MLIRT, MODEL_RTIRT, MODEL_NULL, MODEL_CROSS, MODEL_LATENT)      # the models erm_get_marginal_waic serves (no quantile weights)
QUANTILE_MARGINAL_MODELS = (MODEL_LATENTQR,)      # the model erm_get_quantile_marginal_waic serves (nu integrated out with theta and zeta)
MARGINAL_NODES = 61
# The two families of the marginal WAIC and PSIS-LOO (FAMILY_GAUSSIAN / FAMILY_QUANTILE of csrc/erm_item_pass.hpp): the models a family serves, the stem of its
# Engine / Farm methods and of its erm_get_* / erm_farm_get_* symbols (stem + "waic" | "loo"), its caller-data symbol, and the scalars (doubles) that symbol takes
# between the rows and the node count.
MarginalFamily = namedtuple("MarginalFamily", "models stem loglik scalars")
MARGINAL_FAMILIES = MappingProxyType({
    "gaussian": MarginalFamily(MARGINAL_MODELS, "marginal_", "erm_marginal_loglik", ()),
    "quantile": MarginalFamily(QUANTILE_MARGINAL_MODELS, "quantile_marginal_", "erm_quantile_marginal_loglik", ("q_rt",)),
})


def marginal_nodes(nodes):
    """The node count of the marginal WAIC's theta rule as the library accepts it: odd and in 3 .. 1025 (None or 0: the default, 61)."""
    if nodes is None or nodes == 0:
        return MARGINAL_NODES
    Q = int(nodes)
    if Q != nodes or Q < 3 or Q > 1025 or Q % 2 == 0:
        raise ValueError("nodes must be odd and in 3 .. 1025")
    return Q


def item_trace_width(model, J, F):
    """Columns of an item-trace row: a, b, lambda, sig2t [4][J], then the kernels' small part of qr (item_trace_width of csrc/erm_model.hpp)."""
    t = MODEL_TRAITS[model]
    Fk = kernel_feat(model, F)
    head = J if t.rho else {"none": 0, "vec": Fk + 1, "pair": 2 * (Fk + 1), "latent": Fk + 2, "zero_pair": 2 * (Fk + 1)}[t.beta]
    return 4 * J + head + (4 if t.rt else 0)


def _marginal_result(out, lppd, p):
    res = dict(elpd=float(out[0]), pWaic=float(out[1]), WAIC=float(out[2]), se=float(out[3]), lppd=float(out[4]), nUnits=int(out[5]), nRows=int(out[6]),
               nHighVar=int(out[7]), nNodes=int(out[8]), nCoarse=int(out[9]))
    return (res, lppd, p) if lppd is not None else res


def _marginal_call(fn, h, nodes, n_subj, pointwise):
    out = np.empty(10, dtype=np.float64)
    lppd, p = (np.empty(n_subj), np.empty(n_subj)) if pointwise else (None, None)
    check(fn(h, marginal_nodes(nodes), out.ctypes.data, None if lppd is None else lppd.ctypes.data, None if p is None else p.ctypes.data))
    return _marginal_result(out, lppd, p)


# erm_get_scores / erm_farm_get_scores / erm_score: the columns of score [n_subj][7] (ERM_SCORE_*) and the weightings of the rows
SCORE_COLUMNS = ("theta", "thetaSd", "zeta", "zetaSd", "cov", "rowEss", "coarse")
SCORE_EQUAL, SCORE_LIKELIHOOD = 0, 1
SCORE_WEIGHTINGS = {"equal": SCORE_EQUAL, "likelihood": SCORE_LIKELIHOOD}


def score_weighting(weighting):
    """The weighting of the rows as the library takes it: "equal" | "likelihood" (or the ERM_SCORE_* code)."""
    if weighting in SCORE_WEIGHTINGS:
        return SCORE_WEIGHTINGS[weighting]
    if weighting in (SCORE_EQUAL, SCORE_LIKELIHOOD) and not isinstance(weighting, bool):
        return int(weighting)
    raise ValueError('weighting must be "equal" or "likelihood"')


# erm_get_person_fit / erm_farm_get_person_fit / erm_person_fit: the columns of fit [n_subj][6] (ERM_FIT_*); the weightings are the scores'
FIT_COLUMNS = ("lz", "pResp", "ltz", "pTime", "rowEss", "coarse")


# erm_get_item_fit / erm_farm_get_item_fit / erm_item_fit: the columns of fit [n_item][6] (ERM_IFIT_*)
IFIT_COLUMNS = ("infit", "outfit", "respZ", "rtMsq", "rtZ", "nObs")


# The three passes whose product is one table [n][columns]: the columns, the config field that sizes the table, what the last column -- a count or a flag
# carried as a double -- becomes in the dict, and whether the caller-data entry takes a weighting of the rows
PassTable = namedtuple("PassTable", "columns size last weighted")
PASS_TABLES = MappingProxyType({
    "scores": PassTable(SCORE_COLUMNS, "n_subj", lambda flag: flag != 0.0, True),
    "person_fit": PassTable(FIT_COLUMNS, "n_subj", lambda flag: flag != 0.0, True),
    "item_fit": PassTable(IFIT_COLUMNS, "n_item", lambda count: count.astype(np.int64), False),
})


def _table_buffers(name, n):
    return np.empty((len(PASS_TABLES[name].columns), n), dtype=np.float64), np.empty(4, dtype=np.float64)


def _table_result(name, table, out):
    """table as the library fills it, (columns, n) C-ordered = column-major [n][columns], and out4 -> a dict of the columns with nSubj, nRows, nNodes, nCoarse."""
    t = PASS_TABLES[name]
    res = {column: table[k] for k, column in enumerate(t.columns)}
    res[t.columns[-1]] = t.last(table[-1])
    res.update(nSubj=int(out[0]), nRows=int(out[1]), nNodes=int(out[2]), nCoarse=int(out[3]))
    return res


def _table_call(name, fn, h, nodes, cfg):
    table, out = _table_buffers(name, getattr(cfg, PASS_TABLES[name].size))
    check(fn(h, marginal_nodes(nodes), table.ctypes.data, out.ctypes.data))
    return _table_result(name, table, out)


# erm_get_plausible_values / erm_farm_get_plausible_values / erm_plausible_values: the number of draws, the seed, and the outputs
PV_DRAWS, PV_DRAWS_MAX, PV_SEED, PV_SITE = 5, 4096, 20191, 16


def pv_draws(K):
    """The number of plausible values per subject as the library takes it: 1 .. 4096."""
    if isinstance(K, bool) or K != int(K) or int(K) < 1 or int(K) > PV_DRAWS_MAX:
        raise ValueError(f"K must be an integer in 1 .. {PV_DRAWS_MAX}")
    return int(K)


def pv_seed(seed):
    """The seed of the draws: an integer in 0 .. 2^64 - 1 (the Philox key)."""
    if isinstance(seed, bool) or seed != int(seed) or int(seed) < 0 or int(seed) >= 1 << 64:
        raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
    return int(seed)


def _pv_call(fn, n_subj, K, seed, *head):
    """fn(*head, K, seed, pv, node, coarse, out4) -> a dict: theta, zeta (n_subj, K), node (n_subj, K), coarse (n_subj,) bool, nSubj, nRows, nNodes, nCoarse, seed."""
    K, seed = pv_draws(K), pv_seed(seed)
    pv, node = np.empty((2, K, n_subj), dtype=np.float64), np.empty((K, n_subj), dtype=np.int32)       # C-ordered = column-major [n_subj][K][2], [n_subj][K]
    coarse, out = np.empty(n_subj, dtype=np.int32), np.empty(4, dtype=np.float64)
    check(fn(*head, K, seed, pv.ctypes.data, node.ctypes.data, coarse.ctypes.data, out.ctypes.data))
    return dict(theta=pv[0].T, zeta=pv[1].T, node=node.T, coarse=coarse != 0, nSubj=int(out[0]), nRows=int(out[1]), nNodes=int(out[2]), nCoarse=int(out[3]), seed=seed)


# erm_get_marginal_loo / erm_farm_get_marginal_loo / erm_psis_loo: the columns of pw [n_subj][4] (ERM_LOO_*) and the limits of the rows per unit
LOO_COLUMNS = ("elpd_u", "p_u", "khat", "nEff")
PSIS_MIN_ROWS, PSIS_MAX_ROWS, PSIS_K_BAD = 25, 8192, 0.7


def psis_rows(S):
    """The rows per unit as PSIS-LOO takes them: 25 .. 8192."""
    S = int(S)
    if S < PSIS_MIN_ROWS or S > PSIS_MAX_ROWS:
        raise ValueError(f"PSIS-LOO needs {PSIS_MIN_ROWS} .. {PSIS_MAX_ROWS} rows per unit ({S} given)")
    return S


def _loo_result(out, pw):
    """out12 and pw as the library fills it, (4, n_subj) C-ordered = column-major [n_subj][4], -> a dict of the totals, with the pointwise columns if pw is given."""
    res = dict(elpd=float(out[0]), pLoo=float(out[1]), LOOIC=float(out[2]), se=float(out[3]), lppd=float(out[4]), nUnits=int(out[5]), nRows=int(out[6]),
               nBadK=int(out[7]), nHighK=int(out[8]), tailLen=int(out[9]), nNodes=int(out[10]), nCoarse=int(out[11]))
    if pw is not None:
        res.update({name: pw[k] for k, name in enumerate(LOO_COLUMNS)})
    return res


def _loo_call(fn, h, nodes, n_subj, pointwise):
    out = np.empty(12, dtype=np.float64)
    pw = np.empty((len(LOO_COLUMNS), n_subj), dtype=np.float64) if pointwise else None
    check(fn(h, marginal_nodes(nodes), out.ctypes.data, None if pw is None else pw.ctypes.data))
    return _loo_result(out, pw)


STATE_FIELDS = ("theta", "a", "b", "zeta", "lambda_", "sig2t", "beta", "sigp", "rho", "nu")


def state_struct(arrays: dict):
    """Build an erm_state from {field: float64 contiguous ndarray or None}; returns (struct, keepalive)."""
    st = erm_state()
    keep = []
    for f in STATE_FIELDS:
        v = arrays.get(f)
        if v is None:
            setattr(st, f, None)
        else:
            assert v.dtype == np.float64 and (v.flags["C_CONTIGUOUS"] or v.flags["F_CONTIGUOUS"])
            keep.append(v)
            setattr(st, f, v.ctypes.data_as(_DP))
    return st, keep


class _Diagnostics:
    """The four convergence queries of an Engine (erm_get_*: its own interleaved chains) and of a Farm (erm_farm_get_*: its chains jointly, M = 2 * n_chains split
    sequences, computed on chain 0's device).  One implementation, keyed by the symbol prefix `_get_prefix`; `_diag_width(which)` is the trace's width."""
    _get_prefix = "erm_get_"

    def _diag_width(self, which: int):
        return int(self._lib.erm_trace_width(self._h, which))

    def _diag_vectors(self, name: str, which: int, n: int):
        w = max(self._diag_width(which), 0)
        out = tuple(np.empty(w) for _ in range(n))
        check(getattr(self._lib, self._get_prefix + name)(self._h, which, *(v.ctypes.data for v in out)))
        return out

    def _diag_counts(self, name: str, which: int, n: int):
        c = np.zeros(n, dtype=np.int64)
        check(getattr(self._lib, self._get_prefix + name)(self._h, which, c.ctypes.data))
        return tuple(int(v) for v in c)

    def diagnostics(self, which: int):
        """(ess, rhat) of every column of Post.ra / rt / qr, computed on the device from the resident traces (erm_get_diagnostics / erm_farm_get_diagnostics)."""
        return self._diag_vectors("diagnostics", which, 2)

    def convergence(self, which: int):
        """erm_get_convergence / erm_farm_get_convergence: (columns with a defined ESS, of those ESS > 400, columns with a defined R-hat, of those R-hat < 1.1),
        counted on the device."""
        return self._diag_counts("convergence", which, 4)

    def rank_diagnostics(self, which: int):
        """(ess_bulk, ess_tail, rhat_rank) of every column of Post.ra / rt / qr: the rank-normalised diagnostics (erm_get_rank_diagnostics /
        erm_farm_get_rank_diagnostics), computed on the device from the resident traces."""
        return self._diag_vectors("rank_diagnostics", which, 3)

    def rank_convergence(self, which: int):
        """erm_get_rank_convergence / erm_farm_get_rank_convergence: (bulk-ESS defined, bulk-ESS > 400, tail-ESS defined, tail-ESS > 400, rank R-hat defined,
        rank R-hat < 1.1), counted on the device."""
        return self._diag_counts("rank_convergence", which, 6)


class _ItemPasses:
    """The six passes over the item trace of an Engine (erm_get_*: its resident data set and its own post-burn-in rows) and of a Farm (erm_farm_get_*: the
    post-burn-in rows of all chains -- chain 0's, then chain 1's, ... -- on chain 0's device and data set).  One implementation, keyed by `_get_prefix`."""

    def _pass(self, name: str):
        return getattr(self._lib, self._get_prefix + name)

    def _marginal(self, family: str, product: str, nodes, pointwise):
        """The "waic" or "loo" entry of a family of MARGINAL_FAMILIES."""
        call = {"waic": _marginal_call, "loo": _loo_call}[product]
        return call(self._pass(MARGINAL_FAMILIES[family].stem + product), self._h, nodes, self.cfg.n_subj, pointwise)

    def marginal_waic(self, nodes=MARGINAL_NODES, pointwise=False):
        """erm_get_marginal_waic / erm_farm_get_marginal_waic: WAIC with every subject's theta and zeta integrated out, computed on the device from the resident
        item trace after the run.  The totals (erm_get_waic's, with nNodes and nCoarse); with pointwise=True (totals, lppd_i, p_i)."""
        return self._marginal("gaussian", "waic", nodes, pointwise)

    def marginal_loo(self, nodes=MARGINAL_NODES, pointwise=False):
        """erm_get_marginal_loo / erm_farm_get_marginal_loo: Pareto-smoothed leave-one-subject-out on the marginal log-likelihoods, computed on the device from the
        resident item trace after the run.  Returns a dict of out12; pointwise=True adds elpd_u, p_u, khat, nEff [n_subj]."""
        return self._marginal("gaussian", "loo", nodes, pointwise)

    def quantile_marginal_waic(self, nodes=MARGINAL_NODES, pointwise=False):
        """erm_get_quantile_marginal_waic / erm_farm_get_quantile_marginal_waic: marginal_waic for a LatentQr engine or farm, with the quantile weights integrated
        out too, at its q_rt.  The same outputs."""
        return self._marginal("quantile", "waic", nodes, pointwise)

    def quantile_marginal_loo(self, nodes=MARGINAL_NODES, pointwise=False):
        """erm_get_quantile_marginal_loo / erm_farm_get_quantile_marginal_loo: marginal_loo for a LatentQr engine or farm.  The same outputs."""
        return self._marginal("quantile", "loo", nodes, pointwise)

    def scores(self, nodes=MARGINAL_NODES):
        """erm_get_scores / erm_farm_get_scores: every subject's posterior mean and sd of theta and zeta, their covariance and the rows' effective size, computed on
        the device from the resident item trace after the run (equal weights).  A dict of SCORE_COLUMNS [n_subj] with nSubj, nRows, nNodes, nCoarse."""
        return _table_call("scores", self._pass("scores"), self._h, nodes, self.cfg)

    def person_fit(self, nodes=MARGINAL_NODES):
        """erm_get_person_fit / erm_farm_get_person_fit: every subject's lz with its normal p-value, the Wilson-Hilferty z of the response-time quadratic form with
        its exact chi^2 p-value, and the rows' effective size, computed on the device from the resident item trace after the run (equal weights).  A dict of
        FIT_COLUMNS [n_subj] with nSubj, nRows, nNodes, nCoarse."""
        return _table_call("person_fit", self._pass("person_fit"), self._h, nodes, self.cfg)

    def item_fit(self, nodes=MARGINAL_NODES):
        """erm_get_item_fit / erm_farm_get_item_fit: every item's infit, outfit, signed response residual, response-time mean square and signed response-time
        residual with the number of subjects that observed it, computed on the device from the resident item trace after the run (equal weights).  A dict of
        IFIT_COLUMNS [n_item] with nSubj, nRows, nNodes, nCoarse."""
        return _table_call("item_fit", self._pass("item_fit"), self._h, nodes, self.cfg)

    def plausible_values(self, K=PV_DRAWS, seed=PV_SEED, nodes=MARGINAL_NODES):
        """erm_get_plausible_values / erm_farm_get_plausible_values: K draws of every subject's (theta, zeta) from its posterior given the resident item trace,
        computed on the device after the run.  A dict: theta, zeta (n_subj, K), node (n_subj, K), coarse (n_subj,), nSubj, nRows, nNodes, nCoarse, seed."""
        return _pv_call(self._pass("plausible_values"), self.cfg.n_subj, K, seed, self._h, marginal_nodes(nodes))


class Engine(_Diagnostics, _ItemPasses):
    """Thin RAII wrapper over an erm_handle."""

    def __init__(self, **kw):
        lib = load()
        cfg = erm_config()
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown config field {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self._pw_unit = None         # the WAIC unit as set through this object (None: never; a unit set past it, through the C ABI, is read off the unit count)
        self._h = C.c_void_p()
        check(lib.erm_create(C.byref(cfg), C.byref(self._h)))
        self._lib = lib

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.erm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_shard(self, rank: int, count: int, n_subj_total: int, row_base: int, exchange):
        """Make this engine one shard of a subject-sharded chain (include/ertirt.h, erm_set_shard).  `exchange(send_ptr, recv_ptr,
        nbytes)` is the all-gather over the shards (see parallel.TorchExchange / parallel.ThreadExchange); an exception it raises
        is kept in `self.exchange_error` and surfaces as an ErmError from the call that triggered the exchange."""
        self.exchange_error = None

        def _cb(user, send, recv, nbytes):
            try:
                exchange(send, recv, int(nbytes))
                return 0
            except BaseException as e:      # never let an exception cross the C frames
                self.exchange_error = e
                return -1

        self._exchange_cb = EXCHANGE_FN(_cb)       # kept alive as long as the engine
        check(self._lib.erm_set_shard(self._h, rank, count, n_subj_total, row_base, self._exchange_cb, None))

    def set_shard_rccl(self, rank: int, count: int, n_subj_total: int, row_base: int, unique_id: bytes):
        """Shard with the library's own in-stream RCCL all-gather (erm_set_shard_rccl); `unique_id`: the 128 bytes of rccl_unique_id()
        made on one rank and handed to all of them."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of rccl_unique_id()")
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self._lib.erm_set_shard_rccl(self._h, rank, count, n_subj_total, row_base, buf))

    # ---- data / state
    def set_data(self, Y, logT=None, X=None):
        Ya = np.asarray(Y)
        if Ya.dtype != np.bool_ and not np.all((Ya == 0) | (Ya == 1)):
            raise ValueError("Y must contain only 0/1")
        Yf = np.asfortranarray(Ya.astype(np.uint8))
        lt = None if logT is None else np.asfortranarray(logT, dtype=np.float64)
        xx = None if X is None or np.size(X) == 0 else np.asfortranarray(X, dtype=np.float64)
        check(self._lib.erm_set_data(self._h, Yf.ctypes.data, None if lt is None else lt.ctypes.data,
                                     None if xx is None else xx.ctypes.data))

    def simulate_data(self, seed=4321, noise=0, pull_truth=True, **truth):
        """Generate the data set on the device from the true parameters (erm_simulate_data); returns (theta, zeta) of the truth (None with
        pull_truth=False: they stay on the device, erm_get_truth fetches them later if wanted)."""
        arrs = {k: (None if v is None else np.asfortranarray(v, dtype=np.float64)) for k, v in truth.items()}
        st, keep = state_struct(arrs)
        check(self._lib.erm_simulate_data(self._h, C.byref(st), int(seed), int(noise)))
        if not pull_truth:
            return None
        th, ze = np.empty(self.cfg.n_subj), np.empty(self.cfg.n_subj)
        check(self._lib.erm_get_truth(self._h, th.ctypes.data, ze.ctypes.data))
        return th, ze

    def get_data(self):
        """The resident data set as (Y uint8 NxJ, logT float64 NxJ or None, X float64 NxF or None), column-major."""
        c = self.cfg
        N, J = c.n_subj, c.n_item
        F = kernel_feat(c.model, c.n_feat)
        Y = np.empty((N, J), dtype=np.uint8, order="F")
        logT = np.empty((N, J), dtype=np.float64, order="F") if MODEL_TRAITS[c.model].rt else None
        X = np.empty((N, F), dtype=np.float64, order="F") if F > 0 else None
        check(self._lib.erm_get_data(self._h, Y.ctypes.data, None if logT is None else logT.ctypes.data, None if X is None else X.ctypes.data))
        return Y, logT, X

    def set_state(self, **arrays):
        arrs = {k: (None if v is None else np.asfortranarray(v, dtype=np.float64)) for k, v in arrays.items()}
        st, keep = state_struct(arrs)
        check(self._lib.erm_set_state(self._h, C.byref(st)))

    def _state_buffers(self, which=None):
        c = self.cfg
        N, J, F = c.n_subj, c.n_item, c.n_feat
        sizes = dict(theta=N, a=J, b=J, zeta=N, lambda_=J, sig2t=J, beta=nbeta(c.model, F), sigp=4, rho=J, nu=nu_len(c.model, N, J))
        return {k: (np.zeros(n, dtype=np.float64) if n and (which is None or k in which) else None) for k, n in sizes.items()}

    def get_state(self, which=None):
        bufs = self._state_buffers(which)
        st, keep = state_struct(bufs)
        check(self._lib.erm_get_state(self._h, C.byref(st)))
        return bufs

    def get_mean(self, which=None):
        bufs = self._state_buffers(which)
        st, keep = state_struct(bufs)
        check(self._lib.erm_get_mean(self._h, C.byref(st)))
        return bufs

    # ---- run / outputs
    def run(self, nsweeps: int):
        check(self._lib.erm_run(self._h, int(nsweeps)))

    def reset_trace(self):
        check(self._lib.erm_reset_trace(self._h))

    def set_seed(self, seed: int):
        """A new seed for the chain's random streams (erm_set_seed): one engine serves every replication of a simulation condition."""
        check(self._lib.erm_set_seed(self._h, int(seed)))
        self.cfg.seed = int(seed)

    def dic(self):
        """erm_get_dic: {Dbar, Dhat, pD, DIC} from device-resident state (the log-likelihood at Post.mean is one evaluation pass on the device)."""
        out = np.empty(4, dtype=np.float64)
        check(self._lib.erm_get_dic(self._h, out.ctypes.data))
        return dict(Dbar=float(out[0]), Dhat=float(out[1]), pD=float(out[2]), DIC=float(out[3]))

    # ---- WAIC (erm_set_pointwise / erm_get_waic / erm_get_pointwise)
    def set_pointwise(self, unit):
        """Enable WAIC with unit "subject" or "cell" (or a POINTWISE_* code), None / POINTWISE_OFF turns it off; only while no trace row is recorded."""
        if unit is None or isinstance(unit, str):
            if unit not in POINTWISE_UNITS:
                raise ValueError("waic must be None, 'subject' or 'cell'")
            unit = POINTWISE_UNITS[unit]
        check(self._lib.erm_set_pointwise(self._h, int(unit)))
        self._pw_unit = int(unit)

    @property
    def pointwise_units(self):
        return int(self._lib.erm_pointwise_units(self._h))

    def waic(self):
        """erm_get_waic: the totals, finished and summed on the device."""
        out = np.empty(8, dtype=np.float64)
        check(self._lib.erm_get_waic(self._h, out.ctypes.data))
        return dict(elpd=float(out[0]), pWaic=float(out[1]), WAIC=float(out[2]), se=float(out[3]), lppd=float(out[4]), nUnits=int(out[5]), nRows=int(out[6]),
                    nHighVar=int(out[7]))

    def pointwise(self):
        """erm_get_pointwise: (lppd_u, p_u); subjects in order, cells as an (nSubj, nItem) Fortran-ordered array."""
        U = self.pointwise_units
        lppd, p = np.empty(U, dtype=np.float64), np.empty(U, dtype=np.float64)
        check(self._lib.erm_get_pointwise(self._h, lppd.ctypes.data, p.ctypes.data))
        # (the unit as set through this object; set past it, the count decides -- which cannot tell the units apart at one item, as many cells as subjects: the
        # C ABI has no getter for the unit, and there the two shapes hold the same values in the same order)
        unit = self._pw_unit if self._pw_unit is not None else (POINTWISE_CELL if U != self.cfg.n_subj else POINTWISE_SUBJECT)
        if unit == POINTWISE_CELL and U == self.cfg.n_subj * self.cfg.n_item:
            sh = (self.cfg.n_subj, self.cfg.n_item)
            return lppd.reshape(sh, order="F"), p.reshape(sh, order="F")
        return lppd, p

    # ---- posterior predictive checks (erm_set_predictive / erm_predictive_reps / erm_get_predictive)
    def set_predictive(self, on=True, thin=1):
        """Enable the replicate pass (every thin-th post-burn-in row is replicated) or turn it off; only while no trace row is recorded."""
        check(self._lib.erm_set_predictive(self._h, int(bool(on)), int(thin)))

    @property
    def predictive_reps(self):
        return int(self._lib.erm_predictive_reps(self._h))

    def predictive(self):
        """erm_get_predictive: (item (3, 4, nItem), subj (2, 4, nSubj), total (2, 4)); components RA, RT[, SCORE] x {n_ge, n_gt, mean_obs, mean_rep}."""
        N, J = self.cfg.n_subj, self.cfg.n_item
        item, subj, total = np.empty((3, 4, J)), np.empty((2, 4, N)), np.empty((2, 4))
        check(self._lib.erm_get_predictive(self._h, item.ctypes.data, subj.ctypes.data, total.ctypes.data))
        return item, subj, total

    @property
    def rows_done(self):
        return int(self._lib.erm_rows_done(self._h))

    @property
    def post_count(self):
        return int(self._lib.erm_post_count(self._h))

    def trace(self, which: int):
        """Post.ra / rt / qr / logLike as an (nIter, width, nChain) Fortran-ordered array (Julia layout)."""
        w = int(self._lib.erm_trace_width(self._h, which))
        if w <= 0:
            return np.zeros((0,), dtype=np.float64)
        out = np.empty((self.cfg.n_iter, w, self.cfg.n_chain), dtype=np.float64, order="F")
        check(self._lib.erm_get_trace(self._h, which, out.ctypes.data))
        return out

    def item_trace(self):
        w = int(self._lib.erm_item_trace_width(self._h))
        out = np.empty((self.rows_done, w), dtype=np.float64)
        if out.size:
            check(self._lib.erm_get_item_trace(self._h, out.ctypes.data))
        return out

    def timing(self):
        t = erm_timing()
        check(self._lib.erm_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in erm_timing._fields_}


class _Borrowed(Engine):
    """A farm's engine seen through the Engine wrapper (owned by the farm: never destroyed from here)."""

    def __init__(self, lib, handle, cfg):
        self._lib, self._h, self.cfg = lib, handle, cfg
        self._pw_unit = None

    def close(self):
        self._h = None


class Farm(_Diagnostics, _ItemPasses):
    """erm_farm_*: nChain independent chains, chain l on device devices[l] (include/ertirt.h).  The chains sample concurrently on host
    threads of the library; get_mean() is the one collective (RCCL all-reduce over the devices)."""

    def __init__(self, devices, **kw):
        lib = load()
        cfg = erm_config()
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown config field {k}")
            setattr(cfg, k, v)
        self.cfg, self._lib = cfg, lib
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        check(lib.erm_farm_create(C.byref(cfg), arr, len(self.devices), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.erm_farm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_chains(self):
        return int(self._lib.erm_farm_chains(self._h))

    def engine(self, chain: int):
        h = self._lib.erm_farm_engine(self._h, int(chain))
        if not h:
            raise ErmError("no such chain")
        c = erm_config.from_buffer_copy(self.cfg)
        c.n_chain, c.chain_id, c.device = 1, int(chain), self.devices[chain]
        return _Borrowed(self._lib, C.c_void_p(h), c)

    def set_data(self, Y, logT=None, X=None):
        Ya = np.asarray(Y)
        if Ya.dtype != np.bool_ and not np.all((Ya == 0) | (Ya == 1)):
            raise ValueError("Y must contain only 0/1")
        Yf = np.asfortranarray(Ya.astype(np.uint8))
        lt = None if logT is None else np.asfortranarray(logT, dtype=np.float64)
        xx = None if X is None or np.size(X) == 0 else np.asfortranarray(X, dtype=np.float64)
        check(self._lib.erm_farm_set_data(self._h, Yf.ctypes.data, None if lt is None else lt.ctypes.data, None if xx is None else xx.ctypes.data))

    def set_state(self, chain: int, **arrays):
        arrs = {k: (None if v is None else np.asfortranarray(v, dtype=np.float64)) for k, v in arrays.items()}
        st, keep = state_struct(arrs)
        check(self._lib.erm_farm_set_state(self._h, int(chain), C.byref(st)))

    def get_state(self, chain: int):
        bufs = self.engine(chain)._state_buffers()
        st, keep = state_struct(bufs)
        check(self._lib.erm_farm_get_state(self._h, int(chain), C.byref(st)))
        return bufs

    def run(self, nsweeps: int):
        check(self._lib.erm_farm_run(self._h, int(nsweeps)))

    def reset_trace(self):
        check(self._lib.erm_farm_reset_trace(self._h))

    @property
    def post_count(self):
        return int(self._lib.erm_farm_post_count(self._h))

    @property
    def used_rccl(self):
        return bool(self._lib.erm_farm_used_rccl(self._h))

    def get_mean(self):
        bufs = self.engine(0)._state_buffers()
        st, keep = state_struct(bufs)
        check(self._lib.erm_farm_get_mean(self._h, C.byref(st)))
        return bufs

    def set_seed(self, seed: int):
        check(self._lib.erm_farm_set_seed(self._h, int(seed)))
        self.cfg.seed = int(seed)

    def dic(self):
        """erm_farm_get_dic: Dbar over the rows of all chains, Dhat at the joint Post.mean (reduced over the devices like get_mean)."""
        out = np.empty(4, dtype=np.float64)
        check(self._lib.erm_farm_get_dic(self._h, out.ctypes.data))
        return dict(Dbar=float(out[0]), Dhat=float(out[1]), pD=float(out[2]), DIC=float(out[3]))

    # ---- joint convergence diagnostics and item-trace passes over all chains: _Diagnostics and _ItemPasses over erm_farm_get_*; engine(l).diagnostics(which)
    # stays the diagnostic of chain l alone
    _get_prefix = "erm_farm_get_"

    def _diag_width(self, which: int):
        return int(self._lib.erm_trace_width(self._lib.erm_farm_engine(self._h, 0), which))

    def timing(self):
        """erm_farm_get_timing: wall-clock of the last run / gather, per-chain device time, ranks of the library's RCCL communicator."""
        t = erm_farm_timing()
        run_ms = np.zeros(self.n_chains, dtype=np.float64)
        check(self._lib.erm_farm_get_timing(self._h, C.byref(t), run_ms.ctypes.data))
        out = {f: getattr(t, f) for f, _ in erm_farm_timing._fields_}
        out["run_ms"] = run_ms
        return out

    def item_trace(self):
        """Item-level trace rows in the single-engine order (row m * nChain + l = iteration m of chain l)."""
        per = [self.engine(l).item_trace() for l in range(self.n_chains)]
        out = np.empty((per[0].shape[0] * len(per), per[0].shape[1]), dtype=np.float64)
        for l, t in enumerate(per):
            out[l::len(per)] = t
        return out

    def trace(self, which: int):
        """Post.ra / rt / qr / logLike as (nIter, width, nChain), chain l in slab l."""
        w = int(self._lib.erm_trace_width(self._lib.erm_farm_engine(self._h, 0), which))
        if w <= 0:
            return np.zeros((0,), dtype=np.float64)
        out = np.empty((self.cfg.n_iter, w, self.n_chains), dtype=np.float64, order="F")
        check(self._lib.erm_farm_get_trace(self._h, which, out.ctypes.data))
        return out


def _caller_data(model, Y, logT, X, rows):
    """Caller-supplied data and rows as erm_marginal_loglik / erm_score / erm_plausible_values take them: (Y uint8 [N, J], logT [N, J] or None, X [N, F] or None --
    column-major --, rows [R, item_trace_width] row-major) and (N, J, F, R)."""
    Yf = np.asfortranarray(np.asarray(Y).astype(np.uint8))
    if Yf.ndim != 2:
        raise ValueError("Y must be [subject, item]")
    N, J = Yf.shape
    lt = None if logT is None else np.asfortranarray(logT, dtype=np.float64)
    xx = None if X is None or np.size(X) == 0 else np.asfortranarray(X, dtype=np.float64)
    F = 0 if xx is None else xx.shape[1]
    if (lt is not None and lt.shape != (N, J)) or (xx is not None and xx.shape[0] != N):
        raise ValueError("logT / X do not match Y")
    rr = np.ascontiguousarray(rows, dtype=np.float64)
    if model in MODEL_TRAITS and (rr.ndim != 2 or rr.shape[1] != item_trace_width(model, J, F)):
        raise ValueError(f"rows must be [row, {item_trace_width(model, J, F)}]")
    return (Yf, lt, xx, rr), (N, J, F, rr.shape[0])


def _caller_head(device, model, arrays, dims, obs=None, slot=False):
    """The leading arguments of the caller-data entries: device, model, N, J, F, Y, logT, X, rows, R (the arrays stay the caller's to keep alive); with obs
    (_caller_obs), those of their masked siblings: obs stands between X and rows.  slot: the entry has that argument for complete data too (NULL)."""
    N, J, F, R = dims
    ptr = [None if a is None else a.ctypes.data for a in arrays]
    if obs is not None or slot:
        ptr.insert(3, None if obs is None else obs.ctypes.data)
    return (int(device), int(model), N, J, F, *ptr, R)


def _caller_obs(obs, N, J):
    """The observed mask as the masked entries take it: uint8 [N, J] column-major, and n_obs (N,) int32 for them to fill.  The values are the library's to check."""
    O = np.asfortranarray(np.asarray(obs).astype(np.uint8))
    if O.shape != (N, J):
        raise ValueError("obs does not match Y")
    return O, np.empty(N, dtype=np.int32)


def _caller_entry(name, device, model, arrays, dims, obs, single=False):
    """The obs / no-obs fork of a caller-data pass -> (call, extra).  call(*tail) is the entry `name` (obs None: complete data) or name + "_masked", with
    _caller_head's arguments in front of tail and the masked entry's n_obs behind it; extra is what obs adds to the result, nObs [N].  single (erm_item_fit): one
    entry serves both, obs or NULL, and reports no n_obs.  Only a name that has a "_masked" sibling may come with obs (the quantile family has none)."""
    O, n_obs = (None, None) if obs is None else _caller_obs(obs, dims[0], dims[1])
    head = _caller_head(device, model, arrays, dims, O, slot=single)
    reports = obs is not None and not single
    fn = getattr(load(), name + "_masked" if reports else name)
    last = (n_obs.ctypes.data,) if reports else ()

    def call(*tail):
        keep = O      # head holds only the address of the mask: naming the array here keeps it alive for as long as call can be made
        return fn(*head, *tail, *last)
    return call, (dict(nObs=n_obs) if reports else {})


def _caller_table(name, entry, model, Y, logT, X, rows, device, obs, nodes, weighting="equal", single=False):
    """A pass of PASS_TABLES on caller-supplied data: entry(head, nodes[, weighting], table, out4[, n_obs])."""
    arrays, dims = _caller_data(model, Y, logT, X, rows)
    table, out = _table_buffers(name, dims[0] if PASS_TABLES[name].size == "n_subj" else dims[1])
    call, extra = _caller_entry(entry, device, model, arrays, dims, obs, single)
    check(call(marginal_nodes(nodes), *((score_weighting(weighting),) if PASS_TABLES[name].weighted else ()), table.ctypes.data, out.ctypes.data))
    return dict(_table_result(name, table, out), **extra)


def _family_loglik(family, model, Y, logT, X, rows, scalars, nodes, want_l, want_waic, device, obs=None):
    """The caller-data entry of a family of MARGINAL_FAMILIES, with the family's scalars in the table's order; obs: the Gaussian family's masked sibling (the quantile family has
    none, and quantile_marginal_loglik takes no obs)."""
    arrays, (N, J, F, R) = _caller_data(model, Y, logT, X, rows)
    l = np.empty((N, R), dtype=np.float64, order="F") if want_l else None
    out = np.empty(10, dtype=np.float64) if want_waic else None
    lppd, p = (np.empty(N), np.empty(N)) if want_waic else (None, None)
    ptr = lambda a: None if a is None else a.ctypes.data
    call, extra = _caller_entry(MARGINAL_FAMILIES[family].loglik, device, model, arrays, (N, J, F, R), obs)
    check(call(*(float(s) for s in scalars), marginal_nodes(nodes), ptr(l), ptr(out), ptr(lppd), ptr(p)))
    res = dict(l=l, **extra)
    if want_waic:
        res.update(totals=_marginal_result(out, None, None), lppd=lppd, p=p)
    return res


def marginal_loglik(model, Y, logT, X, rows, *, nodes=MARGINAL_NODES, want_l=True, want_waic=True, device=0, obs=None):
    """erm_marginal_loglik: the marginal WAIC's kernel on caller-supplied data (Y, logT [N, J], X [N, F] or None) and item-trace rows [R, item_trace_width] as
    Engine.item_trace() returns them.  Returns a dict: l [N, R] (every l_i^(s)), and -- with want_waic, which needs R >= 2 -- totals, lppd [N], p [N].
    obs [N, J], 0/1 (None: complete, the call above): erm_marginal_loglik_masked on incomplete patterns; the dict then has nObs [N]."""
    return _family_loglik("gaussian", model, Y, logT, X, rows, (), nodes, want_l, want_waic, device, obs)


def quantile_marginal_loglik(model, Y, logT, X, rows, q_rt, *, nodes=MARGINAL_NODES, want_l=True, want_waic=True, device=0):
    """erm_quantile_marginal_loglik: marginal_loglik for LatentQr rows (Latent's layout) at the quantile level q_rt, nu integrated out.  The same dict."""
    return _family_loglik("quantile", model, Y, logT, X, rows, (q_rt,), nodes, want_l, want_waic, device)


def score(model, Y, logT, X, rows, *, nodes=MARGINAL_NODES, weighting="equal", device=0, obs=None):
    """erm_score: the scores' kernel on caller-supplied data (Y, logT [N, J], X [N, F] or None) and item-trace rows [R, item_trace_width] as Engine.item_trace()
    returns them, R >= 1; weighting "equal" | "likelihood".  Returns Engine.scores' dict.  obs [N, J], 0/1 (None: complete, erm_score): erm_score_masked on
    incomplete patterns; the dict then has nObs [N]."""
    return _caller_table("scores", "erm_score", model, Y, logT, X, rows, device, obs, nodes, weighting)


def person_fit(model, Y, logT, X, rows, *, nodes=MARGINAL_NODES, weighting="equal", device=0, obs=None):
    """erm_person_fit: the person fit's kernel on caller-supplied data (Y, logT [N, J], X [N, F] or None) and item-trace rows [R, item_trace_width] as
    Engine.item_trace() returns them, R >= 1; weighting "equal" | "likelihood".  Returns Engine.person_fit's dict.  obs [N, J], 0/1 (None: complete,
    erm_person_fit): erm_person_fit_masked on incomplete patterns; the dict then has nObs [N]."""
    return _caller_table("person_fit", "erm_person_fit", model, Y, logT, X, rows, device, obs, nodes, weighting)


def item_fit(model, Y, logT, X, rows, *, nodes=MARGINAL_NODES, device=0, obs=None):
    """erm_item_fit: the item fit's kernels on caller-supplied data (Y, logT [N, J], X [N, F] or None) and item-trace rows [R, item_trace_width] as
    Engine.item_trace() returns them, R >= 1.  Returns Engine.item_fit's dict.  obs [N, J], 0/1 (None: complete data, the unmasked kernel): incomplete patterns."""
    return _caller_table("item_fit", "erm_item_fit", model, Y, logT, X, rows, device, obs, nodes, single=True)


def plausible_values(model, Y, logT, X, rows, *, K=PV_DRAWS, seed=PV_SEED, nodes=MARGINAL_NODES, device=0, obs=None):
    """erm_plausible_values: the plausible values' kernel on caller-supplied data (Y, logT [N, J], X [N, F] or None) and item-trace rows [R, item_trace_width] as
    Engine.item_trace() returns them, R >= 1.  Returns Engine.plausible_values' dict.  obs [N, J], 0/1 (None: complete, erm_plausible_values):
    erm_plausible_values_masked on incomplete patterns; the dict then has nObs [N]."""
    arrays, dims = _caller_data(model, Y, logT, X, rows)
    call, extra = _caller_entry("erm_plausible_values", device, model, arrays, dims, obs)
    return dict(_pv_call(call, dims[0], K, seed, marginal_nodes(nodes)), **extra)


def psis_loo(l, *, want_lw=False, device=0):
    """erm_psis_loo: the PSIS-LOO kernel on a caller-supplied table l [N, S] of log-likelihoods (unit, row), as marginal_loglik returns it, 25 <= S <= 8192.
    Returns Engine.marginal_loo's pointwise dict (nNodes = nCoarse = 0), with lw [N, S] -- the smoothed, normalised log-weights -- if want_lw."""
    ll = np.asfortranarray(l, dtype=np.float64)
    if ll.ndim != 2:
        raise ValueError("l must be [unit, row]")
    N, S = ll.shape
    out, pw = np.empty(12, dtype=np.float64), np.empty((len(LOO_COLUMNS), N), dtype=np.float64)
    lw = np.empty((N, S), dtype=np.float64, order="F") if want_lw else None
    check(load().erm_psis_loo(int(device), ll.ctypes.data, N, S, out.ctypes.data, pw.ctypes.data, None if lw is None else lw.ctypes.data))
    res = _loo_result(out, pw)
    if want_lw:
        res["lw"] = lw
    return res


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(load().erm_rccl_unique_id(buf))
    return buf.raw


def debug_sample(which, n, par0=None, par1=None, *, seed=1234, site=15, sweep=1, precision=PREC_F64, device=0):
    lib = load()
    out = np.empty(n, dtype=np.float64)
    p0 = None if par0 is None else np.ascontiguousarray(par0, dtype=np.float64)
    p1 = None if par1 is None else np.ascontiguousarray(par1, dtype=np.float64)
    check(lib.erm_debug_sample(device, precision, which, seed, site, sweep, n,
                               None if p0 is None else p0.ctypes.data, None if p1 is None else p1.ctypes.data, out.ctypes.data))
    return out


def sample_gig(p, a, b, n, *, seed=1234, site=15, sweep=1, device=0):
    """n draws of GIG(p, a, b) on the device (erm_sample_gig; rand(GeneralizedInverseGaussian(p, a, b)) of src/GenInvGaussian.jl)."""
    out = np.empty(int(n), dtype=np.float64)
    check(load().erm_sample_gig(device, seed, site, sweep, int(n), float(p), float(a), float(b), out.ctypes.data))
    return out


def debug_convergence(ess, rhat, *, device=0):
    """erm_debug_convergence: erm_get_convergence's four counts of caller-supplied ess / rhat vectors, counted by the same device code."""
    e, r = np.ascontiguousarray(ess, dtype=np.float64), np.ascontiguousarray(rhat, dtype=np.float64)
    if e.shape != r.shape or e.ndim != 1:
        raise ValueError("ess and rhat must be vectors of one length")
    c = np.zeros(4, dtype=np.int64)
    check(load().erm_debug_convergence(device, e.size, e.ctypes.data, r.ctypes.data, c.ctypes.data))
    return tuple(int(v) for v in c)


def rank_diagnostics_device(x, *, precision=PREC_F64, device=0):
    """erm_debug_rank_diagnostics: (ess_bulk, ess_tail, rhat_rank) of the columns of x[draw, column, chain] (post-burn-in draws) through the kernels
    erm_get_rank_diagnostics runs on an engine's traces.  precision=PREC_F32 rounds x to float first, as an fp32 engine's trace does."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("x must be [draw, column, chain]")
    xf = np.asfortranarray(x)
    n_draw, n_col, n_chain = xf.shape
    bulk, tail, rhat = np.empty(n_col), np.empty(n_col), np.empty(n_col)
    check(load().erm_debug_rank_diagnostics(device, precision, xf.ctypes.data, n_draw, n_col, n_chain, bulk.ctypes.data, tail.ctypes.data, rhat.ctypes.data))
    return bulk, tail, rhat


def debug_diagnostics(x, *, precision=PREC_F64, device=0):
    """erm_debug_diagnostics: (ess, rhat) of the columns of x[draw, column, chain] (post-burn-in draws) through the kernel erm_get_diagnostics runs on an engine's
    traces -- the basic estimator's twin of rank_diagnostics_device.  precision=PREC_F32 rounds x to float first, as an fp32 engine's trace does."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("x must be [draw, column, chain]")
    xf = np.asfortranarray(x)
    n_draw, n_col, n_chain = xf.shape
    ess, rhat = np.empty(n_col), np.empty(n_col)
    check(load().erm_debug_diagnostics(device, precision, xf.ctypes.data, n_draw, n_col, n_chain, ess.ctypes.data, rhat.ctypes.data))
    return ess, rhat


def debug_invwishart(nu, psi, n, *, seed=1234, sweep=1, device=0):
    """n draws of the structural step's 2 x 2 InverseWishart(nu, Psi) (erm_debug_invwishart): an (n, 2, 2) array."""
    psi = np.ascontiguousarray(np.asarray(psi, dtype=np.float64).reshape(2, 2).T).reshape(4)      # vec(Psi), column-major
    out = np.empty((int(n), 4), dtype=np.float64)
    check(load().erm_debug_invwishart(device, int(seed), int(sweep), int(n), float(nu), psi.ctypes.data, out.ctypes.data))
    return out.reshape(int(n), 2, 2).transpose(0, 2, 1)

"""Cost of the rank-normalised convergence diagnostics: host wall time of erm_get_rank_diagnostics and of erm_get_diagnostics for the ra
and rt traces of GibbsRtIrt 100 000 x 50, fp64, full traces, nIter = 1000, nChain = 2 (burn-in 500: S = 1000 used draws per column, 100 100 columns per trace).
usage (on the GPU box, from the repo root): python tools/rank_diag_cost.py LIB [reps]      LIB = a libertirt.so ("-" = the in-tree one)
Drives the C ABI directly, so that a library of the parent commit (without erm_get_rank_diagnostics) gives the yardstick -- erm_get_diagnostics alone -- on the same
box.  Each time is a whole call: scratch allocation, the kernels, the copy of the vectors to the host.  A measurement script, not a test."""
import ctypes as C
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("erm_lib_structs", os.path.join(ROOT, "extendedrtirtmodeling.jl_amd", "_lib.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)

path = sys.argv[1] if len(sys.argv) > 1 else "-"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
lib = C.CDLL(L.LIB_PATH if path == "-" else os.path.abspath(path))
has_rank = hasattr(lib, "erm_get_rank_diagnostics")
N, J, F, T, CH = 100_000, 50, 3, 1000, 2


def chk(rc):
    if rc != 0:
        lib.erm_last_error.restype = C.c_char_p
        raise RuntimeError(lib.erm_last_error().decode())


g = np.random.default_rng(1)
Y = np.asfortranarray((g.uniform(size=(N, J)) < 0.6).astype(np.uint8))
logT = np.asfortranarray(4.0 + 0.5 * g.standard_normal((N, J)))
X = np.asfortranarray(g.standard_normal((N, F)))
cfg = L.erm_config(model=L.MODEL_RTIRT, n_item=J, n_subj=N, n_feat=F, n_iter=T, n_chain=CH, n_burnin=T // 2, cov2one=1, q_rt=0.85, seed=3, precision=L.PREC_F64,
                   trace_mode=L.TRACE_FULL)
h = C.c_void_p()
chk(lib.erm_create(C.byref(cfg), C.byref(h)))
chk(lib.erm_set_data(h, C.c_void_p(Y.ctypes.data), C.c_void_p(logT.ctypes.data), C.c_void_p(X.ctypes.data)))
t0 = time.perf_counter()
chk(lib.erm_run(h, C.c_int64(T * CH)))
print(f"{path}: {T * CH} sweeps of GibbsRtIrt {N} x {J} in {time.perf_counter() - t0:.2f} s", flush=True)
lib.erm_trace_width.restype = C.c_int64
total = {"basic": 0.0, "rank": 0.0}
for name, which in (("ra", L.TRACE_RA), ("rt", L.TRACE_RT)):
    w = int(lib.erm_trace_width(h, which))
    a, b, c = np.empty(w), np.empty(w), np.empty(w)
    for kind in ("basic", "rank"):
        if kind == "rank" and not has_rank:
            continue
        ms = []
        for r in range(reps + 1):                           # the first call loads the kernels
            t0 = time.perf_counter()
            if kind == "basic":
                chk(lib.erm_get_diagnostics(h, which, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)))
            else:
                chk(lib.erm_get_rank_diagnostics(h, which, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data)))
            if r:
                ms.append(1e3 * (time.perf_counter() - t0))
        med = float(np.median(ms))
        total[kind] += med
        print(f"{path:32s} {name} {w:>7d} columns {kind:5s} ms min {min(ms):9.2f} median {med:9.2f} max {max(ms):9.2f}   median first vector {np.nanmedian(a):.1f}", flush=True)
if has_rank:
    print(f"{path:32s} ra + rt: basic {total['basic']:.2f} ms, rank {total['rank']:.2f} ms, ratio {total['rank'] / total['basic']:.2f}", flush=True)
lib.erm_destroy.restype = None
lib.erm_destroy(h)

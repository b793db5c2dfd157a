"""Cost of the posterior predictive pass per replicate row: erm_timing.run_ms of 20-sweep calls, fp64, default geometry, with the pass
off, on (thin 1: every sweep is a replicate row) and with the WAIC subject pass instead, at 100 000 x 50 (GibbsRtIrt, GibbsMlIrt, GibbsRtIrtCrossQr) and 1 000 x 15.
usage (on the GPU box, from the repo root): python tools/predictive_cost.py LIB [reps]      LIB = a libertirt.so ("-" = the in-tree one)
Drives the C ABI directly, so that a library of the parent commit (without erm_set_predictive) can be measured with the pass off on the same box.  A measurement
script, not a test."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("erm_lib_structs", os.path.join(ROOT, "extendedrtirtmodeling.jl_amd", "_lib.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)

path = sys.argv[1] if len(sys.argv) > 1 else "-"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
lib = C.CDLL(L.LIB_PATH if path == "-" else os.path.abspath(path))
has_pred, has_waic = hasattr(lib, "erm_set_predictive"), hasattr(lib, "erm_set_pointwise")
F, K = 3, 20


def chk(rc):
    if rc != 0:
        lib.erm_last_error.restype = C.c_char_p
        raise RuntimeError(lib.erm_last_error().decode())


for N, J, models in ((100_000, 50, ((L.MODEL_RTIRT, "GibbsRtIrt"), (L.MODEL_MLIRT, "GibbsMlIrt"), (L.MODEL_CROSSQR, "GibbsRtIrtCrossQr"))), (1_000, 15, ((L.MODEL_RTIRT, "GibbsRtIrt"),))):
    g = np.random.default_rng(1)
    Y = np.asfortranarray((g.uniform(size=(N, J)) < 0.6).astype(np.uint8))
    logT = np.asfortranarray(4.0 + 0.5 * g.standard_normal((N, J)))
    X = np.asfortranarray(g.standard_normal((N, F)))
    for model, name in models:
        base = None
        for mode in ("off", "ppc", "waic-subject"):
            if (mode == "ppc" and not has_pred) or (mode == "waic-subject" and not has_waic):
                continue
            cfg = L.erm_config(model=model, n_item=J, n_subj=N, n_feat=F, n_iter=K * (reps + 1), n_chain=1, n_burnin=0, cov2one=1, q_rt=0.85, seed=3, precision=L.PREC_F64,
                               trace_mode=L.TRACE_SUMMARY)
            h = C.c_void_p()
            chk(lib.erm_create(C.byref(cfg), C.byref(h)))
            chk(lib.erm_set_data(h, C.c_void_p(Y.ctypes.data), C.c_void_p(logT.ctypes.data) if model != L.MODEL_MLIRT else None, C.c_void_p(X.ctypes.data)))
            if mode == "ppc":
                chk(lib.erm_set_predictive(h, 1, 1))
            elif mode == "waic-subject":
                chk(lib.erm_set_pointwise(h, 1))
            us = []
            for r in range(reps + 1):                       # the first call builds the graphs
                chk(lib.erm_run(h, C.c_int64(K)))
                t = L.erm_timing()
                chk(lib.erm_get_timing(h, C.byref(t)))
                if r:
                    us.append(1e3 * t.run_ms / K)
            lib.erm_destroy.restype = None
            lib.erm_destroy(h)
            med = float(np.median(us))
            base = med if mode == "off" else base
            extra = "" if mode == "off" else f"   pass {med - base:8.2f} us = {(med - base) / base:6.3f} of the sweep (persistent = {t.persistent})"
            print(f"{path:32s} {N:>7d} x {J:<3d} {name:18s} {mode:13s} us/sweep min {min(us):8.2f} median {med:8.2f} max {max(us):8.2f}{extra}", flush=True)

"""Cost of WAIC per sweep: erm_timing.run_ms of 20-sweep calls, 100 000 x 50, fp64, default geometry.
usage (on the GPU box, from the repo root): python tools/waic_cost.py LIB [reps]      LIB = a libertirt.so ("-" = the in-tree one)
Drives the C ABI directly, so that a library of the parent commit (without erm_set_pointwise) can be measured with WAIC off: run it alternately with the in-tree
library on ONE box (tools/waic_cost.sh) -- the repeated parent figures are the box's run-to-run spread."""
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
has_waic = hasattr(lib, "erm_set_pointwise")
N, J, F, K = 100_000, 50, 3, 20
g = np.random.default_rng(1)
Y = np.asfortranarray((g.uniform(size=(N, J)) < 0.6).astype(np.uint8))
logT = np.asfortranarray(4.0 + 0.5 * g.standard_normal((N, J)))
X = np.asfortranarray(g.standard_normal((N, F)))


def chk(rc):
    if rc != 0:
        lib.erm_last_error.restype = C.c_char_p
        raise RuntimeError(lib.erm_last_error().decode())


for model, name in ((L.MODEL_RTIRT, "GibbsRtIrt"), (L.MODEL_CROSSQR, "GibbsRtIrtCrossQr")):
    for unit in (0, 1, 2):
        if unit and (not has_waic or (model == L.MODEL_CROSSQR and unit == 2)):
            continue
        cfg = L.erm_config(model=model, n_item=J, n_subj=N, n_feat=F, n_iter=K * (reps + 1), n_chain=1, n_burnin=0, cov2one=1, q_rt=0.85, seed=3, precision=L.PREC_F64,
                           trace_mode=L.TRACE_SUMMARY)
        h = C.c_void_p()
        chk(lib.erm_create(C.byref(cfg), C.byref(h)))
        chk(lib.erm_set_data(h, C.c_void_p(Y.ctypes.data), C.c_void_p(logT.ctypes.data), C.c_void_p(X.ctypes.data)))
        if unit:
            chk(lib.erm_set_pointwise(h, unit))
        us = []
        for r in range(reps + 1):                       # the first call builds the graphs
            chk(lib.erm_run(h, C.c_int64(K)))
            t = L.erm_timing()
            chk(lib.erm_get_timing(h, C.byref(t)))
            if r:
                us.append(1e3 * t.run_ms / K)
        lib.erm_destroy.restype = None
        lib.erm_destroy(h)
        print(f"{path:36s} {name:18s} waic={('off', 'subject', 'cell')[unit]:8s} us/sweep min {min(us):8.2f} median {float(np.median(us)):8.2f} max {max(us):8.2f}", flush=True)

"""Cost of the item fit: host wall time of the item fit against the person fit and the scores on the same inputs, with the protocol of
tools/person_fit_cost.py -- GibbsRtIrt 100 000 x 50, fp64, 250 rows, Q = 61, equal weights, the best of `reps` calls after a warm-up call, host clock around the
call, which synchronises.
usage (on the GPU box, from the repo root): python tools/item_fit_cost.py [reps] [N]
ONE engine holds the data set and 250 post-burn-in rows: nothing is uploaded, the calls are the kernels and their read-back.  erm_get_scores, erm_get_person_fit
and erm_get_item_fit run in this order (so that a kernel trace of the run lists the dispatches in it, reps + 1 per entry; the item fit's are item_fit_kernel, a
memset and item_fit_block_kernel per chunk, then item_fit_finish_kernel).  A measurement script, not a test."""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("erm_lib_structs", os.path.join(ROOT, "extendedrtirtmodeling.jl_amd", "_lib.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
R, Q, J = 250, 61, 50


def best(f):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        f()
        ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms[1:]), max(ms[1:])          # the first call loads the kernel


eng = L.Engine(model=L.MODEL_RTIRT, n_item=J, n_subj=N, n_feat=0, n_iter=R + 10, n_chain=1, n_burnin=10, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64, trace_mode=0)
g = np.random.default_rng(1)
Y = np.asfortranarray((g.uniform(size=(N, J)) < 0.55).astype(np.uint8))
logT = np.asfortranarray(4.0 + g.normal(0, 0.7, (N, J)))
eng.set_data(Y, logT, None)
g = np.random.default_rng(3)
eng.set_state(theta=g.standard_normal(N), zeta=g.standard_normal(N), beta=np.zeros((1, 2)), sigp=np.eye(2))
eng.run(R + 10)
sc = best(lambda: eng.scores(Q))
pf = best(lambda: eng.person_fit(Q))
it = best(lambda: eng.item_fit(Q))
fit = eng.item_fit(Q)
print(f"engine J {J} N {N} rows {R} Q {Q}: erm_get_scores ms min {sc[0]:8.2f} max {sc[1]:8.2f};  erm_get_person_fit ms min {pf[0]:8.2f} max {pf[1]:8.2f};  "
      f"erm_get_item_fit ms min {it[0]:8.2f} max {it[1]:8.2f};  item fit / scores {it[0] / sc[0]:.3f}, item fit / person fit {it[0] / pf[0]:.3f};  "
      f"infit {fit['infit'].min():.3f} .. {fit['infit'].max():.3f}, RT_MSQ {fit['rtMsq'].min():.3f} .. {fit['rtMsq'].max():.3f}, coarse {fit['nCoarse']}", flush=True)
eng.close()

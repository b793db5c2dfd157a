"""Cost of the person fit: host wall time of the person fit against the scores on the same inputs, with the protocol of DESIGN.md 7h -- GibbsRtIrt
100 000 x 50, fp64, 250 rows, Q = 61, equal weights, the best of `reps` calls after a warm-up call, host clock around the call, which synchronises.
usage (on the GPU box, from the repo root): python tools/person_fit_cost.py [reps] [N]
Cases, in this order (so that a kernel trace of the run lists the dispatches in it, reps + 1 per case and entry):
    engine          erm_get_scores, then erm_get_person_fit, on ONE engine that holds the data set and 250 post-burn-in rows: nothing is uploaded, the calls are the
                    kernels and their read-back
    complete        erm_score / erm_person_fit on caller-supplied data, every cell observed
    masked-2of14    erm_score_masked / erm_person_fit_masked at J = 70, 14 blocks of 5 items, every respondent sees 2 blocks at random (n_i = 10): the block design
                    of DESIGN.md 7m's table
A caller-data call validates, transposes or compacts, and uploads the data set every time; that host part is measured apart by a call with ONE row and Q = 3
(`host+upload`).  A measurement script, not a test."""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
R, Q = 250, 61
lib = L.load()


def chk(rc):
    if rc != 0:
        raise RuntimeError(lib.erm_last_error().decode())


def problem(J, seed):
    """Random GibbsRtIrt rows (no covariates: a b lambda sig2t | beta0 pair | vec Sigma_p) and data, column-major."""
    g = np.random.default_rng(seed)
    rows = np.hstack([g.uniform(0.5, 2.0, (R, J)), g.normal(0, 1, (R, J)), 4.0 + 0.3 * g.normal(0, 1, (R, J)), g.uniform(0.1, 0.6, (R, J)), 0.2 * g.normal(0, 1, (R, 2)),
                      np.tile([1.0, 0.3, 0.3, 0.25], (R, 1))])
    Y = np.asfortranarray((g.uniform(size=(N, J)) < 0.55).astype(np.uint8))
    logT = np.asfortranarray(4.0 + g.normal(0, 0.7, (N, J)))
    return np.ascontiguousarray(rows), Y, logT, g


def best(f):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        f()
        ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms[1:]), max(ms[1:])          # the first call loads the kernel


def engine_case():
    """An engine sampled for R post-burn-in rows on simulated data; the two entries read the same resident rows."""
    eng = L.Engine(model=L.MODEL_RTIRT, n_item=50, n_subj=N, n_feat=0, n_iter=R + 10, n_chain=1, n_burnin=10, cov2one=1, q_rt=0.5, seed=1, precision=L.PREC_F64,
                   trace_mode=0)
    g = np.random.default_rng(3)
    rows, Y, logT, _ = problem(50, 1)
    eng.set_data(Y, logT, None)
    eng.set_state(theta=g.standard_normal(N), zeta=g.standard_normal(N), beta=np.zeros((1, 2)), sigp=np.eye(2))
    eng.run(R + 10)
    sc = best(lambda: eng.scores(Q))
    pf = best(lambda: eng.person_fit(Q))
    fit = eng.person_fit(Q)
    print(f"engine        J  50 rows {R}: erm_get_scores ms min {sc[0]:8.2f} max {sc[1]:8.2f};  erm_get_person_fit ms min {pf[0]:8.2f} max {pf[1]:8.2f};  ratio {pf[0] / sc[0]:.3f};  "
          f"flagged pResp {np.mean(fit['pResp'] < 0.05):.4f} pTime {np.mean(fit['pTime'] < 0.05):.4f}, coarse {fit['nCoarse']}", flush=True)
    eng.close()


def call(entry, J, rows, Y, logT, obs, n_rows, nodes):
    cols = 7 if entry == "score" else 6
    res, out4 = np.empty((cols, N)), np.empty(4)
    p = lambda a: C.c_void_p(a.ctypes.data)
    head = (0, L.MODEL_RTIRT, C.c_int64(N), J, 0, p(Y), p(logT), None)
    tail = (p(rows), C.c_int64(n_rows), nodes, 0, p(res), p(out4))
    plain, masked = (lib.erm_score, lib.erm_score_masked) if entry == "score" else (lib.erm_person_fit, lib.erm_person_fit_masked)
    chk(plain(*head, *tail) if obs is None else masked(*head, p(obs), *tail, None))


def case(name, J, rows, Y, logT, obs):
    t = {}
    for entry in ("score", "fit"):
        whole = best(lambda: call(entry, J, rows, Y, logT, obs, R, Q))
        host = best(lambda: call(entry, J, rows, Y, logT, obs, 1, 3))
        t[entry] = whole[0] - host[0]
        print(f"{name:13s} J {J:3d} {entry:5s}: whole call ms min {whole[0]:8.2f} max {whole[1]:8.2f};  host+upload ms min {host[0]:7.2f};  difference {t[entry]:8.2f}", flush=True)
    print(f"{name:13s} person fit / scores, host part taken out: {t['fit'] / t['score']:.3f}", flush=True)


engine_case()
rows, Y, logT, g = problem(50, 1)
case("complete", 50, rows, Y, logT, None)
rows, Y, logT, g = problem(70, 2)
blocks = np.argsort(g.uniform(size=(N, 14)), axis=1)[:, :2]                          # two distinct blocks per respondent
seen = np.zeros((N, 14), dtype=np.uint8)
np.put_along_axis(seen, blocks, 1, axis=1)
case("masked-2of14", 70, rows, Y, logT, np.asfortranarray(np.repeat(seen, 5, axis=1)))

"""Cost of scoring incomplete response patterns: host wall time of erm_score and erm_score_masked on caller-supplied data with the
protocol of DESIGN.md 7h -- GibbsRtIrt 100 000 x 50, fp64, 250 rows, Q = 61, equal weights, the best of `reps` calls after a warm-up call, host clock around the
call, which synchronises.
usage (on the GPU box, from the repo root): python tools/incomplete_cost.py LIB [reps]      LIB = a libertirt.so ("-" = the in-tree one)
Cases, in this order (so that a kernel trace of the run lists score_kernel's dispatches in it, reps + 1 per case):
    complete        erm_score, every cell observed (a library without erm_score_masked runs this case alone: the parent's yardstick on the same box)
    masked-all      erm_score_masked, obs all ones: the price of the indirection
    masked-25       erm_score_masked, 25 % of the cells observed at random
    complete-70     erm_score at J = 70
    masked-2of14    erm_score_masked at J = 70, 14 blocks of 5 items, every respondent sees 2 blocks at random (n_i = 10)
A caller-data call validates, transposes or compacts, and uploads the data set every time; that host part is measured apart by a call with ONE row and Q = 3
(`host+upload`: the kernel's share of it is below a millisecond).  A measurement script, not a test."""
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
lib = C.CDLL(L.LIB_PATH if path == "-" else os.path.abspath(path))
lib.erm_last_error.restype = C.c_char_p
has_masked = hasattr(lib, "erm_score_masked")
N, R, Q = 100_000, 250, 61


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


def call(J, rows, Y, logT, obs, n_rows, nodes):
    score, out4 = np.empty((7, N)), np.empty(4)
    p = lambda a: C.c_void_p(a.ctypes.data)
    head = (0, L.MODEL_RTIRT, C.c_int64(N), J, 0, p(Y), p(logT), None)
    tail = (p(rows), C.c_int64(n_rows), nodes, 0, p(score), p(out4))
    t0 = time.perf_counter()
    chk(lib.erm_score(*head, *tail) if obs is None else lib.erm_score_masked(*head, p(obs), *tail, None))
    return 1e3 * (time.perf_counter() - t0), score


def case(name, J, rows, Y, logT, obs):
    whole = [call(J, rows, Y, logT, obs, R, Q) for _ in range(reps + 1)][1:]              # the first call loads the kernel
    host = [call(J, rows, Y, logT, obs, 1, 3)[0] for _ in range(reps + 1)][1:]
    ms, score = [w[0] for w in whole], whole[0][1]
    cells = N * J if obs is None else int(obs.sum())
    print(f"{path:24s} {name:13s} J {J:3d} observed cells {cells:>9d}: whole call ms min {min(ms):8.2f} max {max(ms):8.2f};  host+upload ms min {min(host):7.2f};  "
          f"difference {min(ms) - min(host):8.2f};  mean theta_sd {np.mean(score[1]):.4f}, coarse {int(np.sum(score[6]))}", flush=True)
    return score


rows, Y, logT, g = problem(50, 1)
ref = case("complete", 50, rows, Y, logT, None)
if has_masked:
    same = case("masked-all", 50, rows, Y, logT, np.ones((N, 50), dtype=np.uint8, order="F"))
    print(f"{'':24s} masked-all equals complete bit for bit: {np.array_equal(same, ref, equal_nan=True)}", flush=True)
    case("masked-25", 50, rows, Y, logT, np.asfortranarray((g.uniform(size=(N, 50)) < 0.25).astype(np.uint8)))
rows, Y, logT, g = problem(70, 2)
case("complete-70", 70, rows, Y, logT, None)
if has_masked:
    blocks = np.argsort(g.uniform(size=(N, 14)), axis=1)[:, :2]                          # two distinct blocks per respondent
    seen = np.zeros((N, 14), dtype=np.uint8)
    np.put_along_axis(seen, blocks, 1, axis=1)
    case("masked-2of14", 70, rows, Y, logT, np.asfortranarray(np.repeat(seen, 5, axis=1)))

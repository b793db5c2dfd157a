#!/usr/bin/env python3
"""Cost of the chain farm's joint convergence diagnostics (GPU box): the wall time of erm_farm_get_rank_convergence(RA) against the host round
trip it replaces, erm_farm_get_trace(RA) + erm_debug_rank_diagnostics on the post-burn-in rows.  A 4-chain farm of GibbsRtIrt 100 000 x 50 on one GPU, fp64,
n_iter = 200, n_burnin = 100.  Every timed call ends in a device synchronise inside the library; one untimed call of each kind comes first.  Prints one JSON line.

usage: python tools/farm_diag_cost.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_util as pu  # noqa: E402
import rank_diag_util as ru  # noqa: E402

N, J, N_ITER, N_BURN, CHAINS = 100_000, 50, 200, 100, 4


def timed_ms(fn, reps):
    """(the last result, the wall time of each of `reps` calls in ms)"""
    times, result = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        result = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return result, times


def make_farm(L):
    Y, logT, X, init = pu.make_problem("rtirt", N, J, 3)[:4]
    farm = L.Farm([0] * CHAINS, model=pu.MODELS["rtirt"], n_item=J, n_subj=N, n_feat=3, n_iter=N_ITER, n_chain=1, n_burnin=N_BURN, cov2one=1, q_rt=0.85,
                  seed=1234, precision=L.PREC_F64, trace_mode=L.TRACE_FULL)
    farm.set_data(Y, logT, X)
    state = {("lambda_" if k == "lam" else k): v for k, v in init.items()}
    for l in range(CHAINS):
        farm.set_state(l, **state)
    farm.run(N_ITER)
    return farm


def main():
    L = pu.ge.load_package()._lib
    farm = make_farm(L)
    which = L.TRACE_RA

    def host_round_trip():
        return L.rank_diagnostics_device(farm.trace(which)[N_BURN:])

    # warm-up: code objects, the rank kernel's LDS attribute
    farm.rank_convergence(which)
    farm.convergence(which)
    counts6, t_rank = timed_ms(lambda: farm.rank_convergence(which), 5)
    counts4, t_basic = timed_ms(lambda: farm.convergence(which), 5)
    os.environ["ERM_FARM_DIAG_REMOTE"] = "1"          # every chain but chain 0 through the slab path
    try:
        counts6_slab, t_slab = timed_ms(lambda: farm.rank_convergence(which), 3)
    finally:
        del os.environ["ERM_FARM_DIAG_REMOTE"]
    (bulk, tail, rhat), t_host = timed_ms(host_round_trip, 2)
    same = ru.counts6(bulk, tail, rhat) == counts6 == counts6_slab
    print(json.dumps(dict(shape=[N, J], chains=CHAINS, n_iter=N_ITER, n_burnin=N_BURN, columns=int(bulk.size), rank_convergence_ms=t_rank,
                          basic_convergence_ms=t_basic, rank_convergence_slab_path_ms=t_slab, host_round_trip_ms=t_host, counts6=list(counts6),
                          counts4=list(counts4), host_counts_equal=bool(same))))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

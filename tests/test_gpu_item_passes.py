"""The two refusals the six item-trace passes share through their one host path (csrc/erm_item_pass.hpp), on the first four of the table -- the
marginal WAIC and LOO, the scores, the plausible values --, for whose entries no other test reaches them; each pass from the engine's and from the farm's entry:
  - an engine without a data set: ERM_ERR_STATE (-3), "no data set is resident";
  - a farm whose chains have recorded different numbers of rows (one chain's borrowed engine ran a sweep further): -3, "rows recorded where chain 0 has".
After either refusal the engine or the farm runs on, and the same call succeeds.
rtirt, 70 subjects (two full tiles of 32 and a tail of 6), 5 items, 1 covariate, 30 iterations of which 2 are burn-in: the 25 rows of the marginal LOO are there."""
import pytest

import parity_util as pu
from test_gpu_marginal_waic import _farm

pytestmark = pytest.mark.gpu

N, J, F, N_ITER, N_BURNIN = 70, 5, 1, 30, 2
PASSES = {"marginal_waic": lambda s: s.marginal_waic(), "marginal_loo": lambda s: s.marginal_loo(), "scores": lambda s: s.scores(),
          "plausible_values": lambda s: s.plausible_values(3, 11)}


@pytest.fixture(scope="module")
def problem():
    return pu.make_problem("rtirt", N, J, F, seed=53)


@pytest.mark.parametrize("name", list(PASSES))
def test_engine_without_a_data_set_refuses_then_serves(problem, name):
    L = pu.ge.load_package()._lib
    Y, logT, X, init, tp = problem
    eng = L.Engine(model=pu.MODELS["rtirt"], n_item=J, n_subj=N, n_feat=F, n_iter=N_ITER, n_chain=1, n_burnin=N_BURNIN, cov2one=1, q_rt=0.85, seed=1234,
                   precision=L.PREC_F64, trace_mode=0)
    with pytest.raises(L.ErmError, match=r"error -3: no data set is resident"):
        PASSES[name](eng)
    eng.set_data(Y, logT, X)
    eng.set_state(**{("lambda_" if k == "lam" else k): v for k, v in init.items()})
    eng.run(N_ITER)
    assert PASSES[name](eng)["nRows"] == N_ITER - N_BURNIN
    eng.close()


@pytest.mark.parametrize("name", list(PASSES))
def test_farm_with_unequal_row_counts_refuses_then_serves(problem, name):
    L = pu.ge.load_package()._lib
    Y, logT, X, init, tp = problem
    farm = _farm("rtirt", [0, 0], Y, logT, X, init, n_iter=N_ITER, n_burnin=N_BURNIN)
    farm.run(N_ITER - 1)
    farm.engine(1).run(1)
    with pytest.raises(L.ErmError, match=rf"error -3: chain 1: {N_ITER} rows recorded where chain 0 has {N_ITER - 1}"):
        PASSES[name](farm)
    farm.engine(0).run(1)
    assert PASSES[name](farm)["nRows"] == 2 * (N_ITER - N_BURNIN)
    farm.close()

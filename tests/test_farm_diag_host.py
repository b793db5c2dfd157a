"""The chain farm's joint convergence diagnostics on the CPU (the device side: tests/test_gpu_farm_diagnostics.py).
  - The chunk arithmetic (extendedrtirtmodeling.jl_amd/csrc/erm_farm_diag.hpp): the header the library includes is compiled by g++ with UndefinedBehaviorSanitizer
    into tests/farm_diag_check.cpp, which sweeps ncol in {1, 31, 32, 33, 316, 1e8} x L in {1, 2, 16} x Tn in {8, 9, 4096} x both element sizes x caps {0, 1, 100}
    (x four budgets) and checks that the chunks cover every column exactly once and that none exceeds the budget unless a single column does.  The plans it
    prints are checked here once more against a restatement in Python integers.
  - checkConvergence's routing: a sampler whose `.farm` is set reads the farm's four methods, for both kinds and with detail on and off, and never its `_engine`.
  - The five new entry points are in _lib.EXPORTS and declared in include/ertirt.h."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import parity_util as pu

pkg = pu.ge.load_package()
SRC = os.path.join(pu.ROOT, "tests", "farm_diag_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")
NEW = ("erm_farm_get_diagnostics", "erm_farm_get_convergence", "erm_farm_get_rank_diagnostics", "erm_farm_get_rank_convergence", "erm_debug_diagnostics")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fd") / "farm_diag_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def test_chunk_arithmetic_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(re.search(r"plans (\d+)", r.stdout).group(1)) == 6 * 3 * 3 * 2 * 3 * 4


def _plan(exe, ncol, Tn, L, elem, budget, cap):
    r = subprocess.run([exe] + [str(v) for v in (ncol, Tn, L, elem, budget, cap)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    return rows[0], rows[1:]


@pytest.mark.parametrize("ncol,Tn,L,elem,budget,cap", [
    (316, 20, 3, 4, 256 << 20, 100), (316, 20, 3, 8, 256 << 20, 1), (316, 20, 16, 8, 256 << 20, 0), (33, 9, 2, 8, 4096, 0), (33, 9, 2, 4, 16, 0), (31, 8, 1, 4, 1000, 100),
    (1, 8, 1, 8, 256 << 20, 0), (100_001, 50, 4, 8, 256 << 20, 0), (100_001, 100, 4, 8, 256 << 20, 0), (302, 20, 3, 4, 256 << 20, 0), (302, 20, 3, 4, 256 << 20, 301), (100_000_000, 4096, 16, 8, 256 << 20, 0), (100_000_000, 8, 1, 4, 256 << 20, 0)])
def test_printed_plan_equals_the_restatement(exe, ncol, Tn, L, elem, budget, cap):
    """The chunk length in Python's unbounded integers: the most columns whose Tn * L * elem bytes each fit the budget (at least one), no more than the cap and
    the block, four or more rounded down to a multiple of four unless the chunk holds the whole block; the list walks the block in steps of it."""
    (chunk, count), rows = _plan(exe, ncol, Tn, L, elem, budget, cap)
    want = budget // (Tn * L * elem)
    if cap > 0:
        want = min(want, cap)
    want = min(want, ncol)
    if 4 <= want < ncol:
        want -= want % 4
    want = max(want, 1)
    assert chunk == want and count == -(-ncol // want)
    assert chunk * Tn * L * elem <= budget or chunk == 1
    starts = list(range(count)) if count <= 2000 else list(range(1000)) + list(range(count - 1000, count))
    assert rows == [(i * chunk, min(chunk, ncol - i * chunk)) for i in starts]
    if count <= 2000:
        assert sum(nc for _, nc in rows) == ncol and rows[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(rows, rows[1:]))
    assert rows[-1][0] + rows[-1][1] == ncol


class _NoEngine:
    """stands where MCMC._engine is: any use of it is a failure"""

    def __getattr__(self, name):
        raise AssertionError(f"checkConvergence touched _engine.{name} although a farm is set")

    def __bool__(self):
        raise AssertionError("checkConvergence looked at _engine although a farm is set")


def _stub_farm(has_rt):
    L = pkg._lib
    nan = float("nan")
    basic = {L.TRACE_RA: (np.array([500.0, 300.0, nan, 401.0]), np.array([1.0, 1.2, nan, 1.05])),
             L.TRACE_RT: (np.array([1000.0, 10.0]), np.array([1.01, 1.5])),
             L.TRACE_QR: (np.array([nan, 450.0, -8.0]), np.array([nan, 1.0999, 1.1]))}
    rank = {L.TRACE_RA: (np.array([500.0, 300.0, nan, 401.0]), np.array([450.0, nan, nan, 399.0]), np.array([1.0, 1.2, nan, 1.05])),
            L.TRACE_RT: (np.array([1000.0, 10.0]), np.array([900.0, 20.0]), np.array([1.01, 1.5])),
            L.TRACE_QR: (np.array([nan, 450.0, -8.0]), np.array([nan, 400.5, 3.0]), np.array([nan, 1.0999, 1.1]))}
    calls = []

    def c4(which):
        e, r = basic[which]
        with np.errstate(invalid="ignore"):
            return (int(np.sum(~np.isnan(e))), int(np.sum(e > 400)), int(np.sum(~np.isnan(r))), int(np.sum(r < 1.1)))

    def c6(which):
        b, t, r = rank[which]
        with np.errstate(invalid="ignore"):
            return (int(np.sum(~np.isnan(b))), int(np.sum(b > 400)), int(np.sum(~np.isnan(t))), int(np.sum(t > 400)), int(np.sum(~np.isnan(r))), int(np.sum(r < 1.1)))

    def rec(name, fn):
        def call(which):
            assert has_rt or which != L.TRACE_RT
            calls.append((name, which))
            return fn(which)
        return call

    farm = types.SimpleNamespace(diagnostics=rec("diagnostics", lambda w: basic[w]), convergence=rec("convergence", c4),
                                 rank_diagnostics=rec("rank_diagnostics", lambda w: rank[w]), rank_convergence=rec("rank_convergence", c6), close=lambda: None)
    return farm, basic, rank, calls


@pytest.mark.parametrize("name,has_rt", [("GibbsRtIrt", True), ("GibbsMlIrt", False)])
def test_check_convergence_reads_the_farm_and_never_the_engine(name, has_rt):
    L = pkg._lib
    M = getattr(pkg, name)(pkg.setCond(nSubj=10, nItem=3, nFeat=1, nIter=4, nChain=2))
    farm, basic, rank, calls = _stub_farm(has_rt)
    M.farm, M._engine = farm, _NoEngine()
    try:
        traces = [("ra", L.TRACE_RA)] + ([("rt", L.TRACE_RT)] if has_rt else []) + [("qr", L.TRACE_QR)]
        # basic: ra 3 defined, 2 above 400 | 3 defined, 2 below 1.1;  rt 2, 1 | 2, 1;  qr 2 (the negative ESS is defined), 1 | 2, 1 (1.1 is not below 1.1)
        want = dict(ess_ok=2 + has_rt + 1, ess_n=3 + 2 * has_rt + 2, rhat_ok=2 + has_rt + 1, rhat_n=3 + 2 * has_rt + 2)
        for detail in (True, False):
            del calls[:]
            res = pkg.checkConvergence(M, detail=detail)
            assert res["essN"] == f"{want['ess_ok']} / {want['ess_n']}" and res["rhatN"] == f"{want['rhat_ok']} / {want['rhat_n']}"
            assert res["ess"] == 100.0 * want["ess_ok"] / want["ess_n"] and res["rhat"] == 100.0 * want["rhat_ok"] / want["rhat_n"]
            assert calls == [("diagnostics" if detail else "convergence", w) for _, w in traces]
            assert ("detail" in res) == detail and set(res) == {"ess", "rhat", "essN", "rhatN"} | ({"detail"} if detail else set())
            if detail:
                assert set(res["detail"]) == {n for n, _ in traces}
                for n, w in traces:
                    assert res["detail"][n][0] is basic[w][0] and res["detail"][n][1] is basic[w][1]
        # rank: bulk as the basic ESS; tail ra 2 defined, 1 above | rt 2, 1 | qr 2, 1 (400.5)
        for detail in (True, False):
            del calls[:]
            res = pkg.checkConvergence(M, kind="rank", detail=detail)
            tail_ok, tail_n = 1 + has_rt + 1, 2 + 2 * has_rt + 2
            assert res["essN"] == f"{want['ess_ok']} / {want['ess_n']}" and res["essTailN"] == f"{tail_ok} / {tail_n}" and res["rhatN"] == f"{want['rhat_ok']} / {want['rhat_n']}"
            assert res["essTail"] == 100.0 * tail_ok / tail_n and res["ess"] == 100.0 * want["ess_ok"] / want["ess_n"]
            assert calls == [("rank_diagnostics" if detail else "rank_convergence", w) for _, w in traces]
            assert ("detail" in res) == detail
            if detail:
                for n, w in traces:
                    assert all(a is b for a, b in zip(res["detail"][n], rank[w]))
        with pytest.raises(ValueError, match="kind must be"):
            pkg.checkConvergence(M, kind="folded")
    finally:
        M.farm, M._engine = None, None
    with pytest.raises(ValueError, match="run sample"):
        pkg.checkConvergence(M)
    with pytest.raises(ValueError, match="run sample"):
        pkg.checkConvergence(M, kind="rank")


def test_new_entry_points_are_exported_and_declared():
    L = pkg._lib
    header = open(os.path.join(pu.ROOT, "include", "ertirt.h")).read()
    for name in NEW:
        assert name in L.EXPORTS and hasattr(L.load(), name), name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
    assert re.search(r"#define ERM_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4
    for method in ("diagnostics", "convergence", "rank_diagnostics", "rank_convergence"):
        assert callable(getattr(L.Farm, method))
    assert callable(L.debug_diagnostics)

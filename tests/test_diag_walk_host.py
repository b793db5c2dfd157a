"""The convergence diagnostics' host path on the CPU (the device side: tests/test_gpu_diagnostics.py, test_gpu_rank_diagnostics.py, test_gpu_farm_diagnostics.py).
The plain-C++ half of extendedrtirtmodeling.jl_amd/csrc/erm_diagnostics.hpp -- the walk over a trace's blocks, the in-place and the gathered source, the limits --
is compiled by g++ with UndefinedBehaviorSanitizer and -ftrapv into tests/diag_walk_check.cpp, which drives the walk with an executor of counters over the seven
models x the three traces x both estimators x an engine of 3 and of 1 chains and farms of 1, 3 and 16 chains x chunk caps 0, 1, 100 x three shapes (N = 37, J = 5
among them: CrossQr's 185-column nu block) x both precisions, and checks that
  - every column of the trace is written exactly once, by one estimate or (constant columns only) by one NaN fill, after one drain and one allocation;
  - an engine is read in place (no gather, the views are its blocks as they stand), a farm chunk by chunk (one gather per estimate, L chains without burn-in);
  - a broken precondition is refused with its code and text before any device operation, and where two are broken the earlier one is reported;
  - diag_limits gives the verdict of the rule it replaced on Tn 0 .. 20 x chains 0 .. 20 and around the cap of 8192 used draws.
The limits are checked here once more against a restatement in Python."""
import os
import re
import subprocess

import pytest

import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "diag_walk_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dw") / "diag_walk_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, "-I", os.path.join(pu.ROOT, "include"),
                    SRC, "-o", out], check=True)
    return out


def test_walk_covers_every_column_once_and_refuses_before_any_device_work(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    walks, refusals, limits = (int(v) for v in re.search(r"walks (\d+) refusals (\d+) limits (\d+)", r.stdout).groups())
    assert walks == 7 * 3 * 2 * 5 * 3 * 3 * 2 and refusals > 7 * 2 * 5 * 6 and limits == 2 * (21 * 21 + 4 * 8)


@pytest.mark.parametrize("rank,Tn,chains,want", [
    (0, 8, 1, None), (0, 7, 1, "too few post-burn-in"), (1, 9, 16, None), (0, 8, 17, "too many chains"), (1, 8, 0, "too many chains"), (0, 7, 17, "too few post-burn-in"),
    (1, 8192, 1, None), (1, 8193, 1, None), (1, 8194, 1, "8192"), (0, 8194, 1, None), (1, 512, 16, None), (1, 514, 16, "8192"), (0, 514, 16, None), (1, 6, 16, "too few post-burn-in")])
def test_limits_name_the_refusal(exe, rank, Tn, chains, want):
    """>= 8 rows after burn-in, then 1 .. 16 chains, then (rank only) at most 8192 used draws 2 * chains * floor(Tn / 2): the first that fails is the one named."""
    r = subprocess.run([exe, "limits", str(rank), str(Tn), str(chains)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    rule = "too few post-burn-in" if Tn // 2 < 4 else "too many chains" if not 1 <= chains <= 16 else "8192" if rank and 2 * chains * (Tn // 2) > 8192 else None
    assert rule == want
    assert (r.stdout.strip() == "ok") if want is None else (want in r.stdout), r.stdout

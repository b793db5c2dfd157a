"""The pure parts of the rank-normalised diagnostics (extendedrtirtmodeling.jl_amd/csrc/erm_rankdiag.hpp) on the CPU: the header the rank kernel includes is compiled
by g++ with UndefinedBehaviorSanitizer into tests/rankdiag_check.cpp, which checks
  - the order-preserving key of a double: strictly increasing over -inf ... +inf through the largest, the smallest normal and the subnormal values, -0.0 and +0.0
    tied, the padding key above +inf, and order and equality kept over two million random bit patterns (neighbours included);
  - the average rank of a tie run against the mean of its positions in long double;
  - the rank -> probability map (inside (0, 1), increasing, symmetric, exactly the three stated operations), k = ceil(S / 20) and the padded length.
The program's ranking (sort by key, walk the tie runs: the device's way) is compared here with scipy.stats.rankdata."""
import os
import subprocess

import numpy as np
import pytest
from scipy.stats import rankdata

import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "rankdiag_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rk") / "rankdiag_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def test_pure_parts_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def _ranks(exe, vals):
    r = subprocess.run([exe, "rank"] + [repr(float(v)) for v in vals], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    return np.array([float(v) for v in r.stdout.split()])


@pytest.mark.parametrize("kind", ["continuous", "ties", "zeros_and_infinities", "constant"])
def test_ranks_equal_scipy_rankdata(exe, kind):
    rng = np.random.default_rng(3)
    x = {"continuous": rng.standard_cauchy(777), "ties": np.floor(2.0 * rng.standard_normal(500)),
         "zeros_and_infinities": rng.choice([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf], 300), "constant": np.full(64, 0.1)}[kind]
    assert np.array_equal(_ranks(exe, x), rankdata(x, method="average"))


def test_keys_of_the_zeros(exe):
    key = lambda v: subprocess.run([exe, "key", v], capture_output=True, text=True, check=True).stdout.strip()
    assert key("-0.0") == key("0.0") == "8000000000000000"
    assert key("-inf") == "000fffffffffffff" and key("inf") == "fff0000000000000"

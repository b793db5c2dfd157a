"""The streaming WAIC accumulators (extendedrtirtmodeling.jl_amd/csrc/erm_pointwise.hpp) on the CPU: the header the pointwise kernel includes is compiled by g++
with UndefinedBehaviorSanitizer into tests/pointwise_check.cpp, which applies pw_update row by row and compares pw_lppd / pw_var with the two-pass evaluation
of the same definition in long double:
  - random sequences of 2 ... 2 000 rows, each also with its maximum moved to the last and to the first row, and ramps in which every row / no row is a new maximum;
  - sequences spanning -700 ... 0;
  - constant sequences: p_u exactly 0 and lppd_u exactly l.
Agreement to 1e-12 relative.  The sample variance of values with mean c and standard deviation sd has condition number ~ |c| / sd with respect to the rounding of
its own inputs (2^-53 relative each), which no algorithm in double can beat; the random sequences and ramps are therefore drawn with sd >= |c| / 10, where the
inputs' rounding alone stays two orders below 1e-12 after 2 000 rows."""
import os
import subprocess

import pytest

import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "pointwise_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pw") / "pointwise_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out], check=True)
    return out


def test_streaming_equals_two_pass_without_undefined_behaviour(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "failures 0" in r.stdout and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def _seq(exe, vals):
    r = subprocess.run([exe, "seq"] + [repr(float(v)) for v in vals], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: float(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


def test_known_answers(exe):
    import math
    d = _seq(exe, [math.log(0.25), math.log(0.75)])           # mean of exp = 1/2, variance = log(3)^2 / 2
    assert abs(d["lppd"] - math.log(0.5)) <= 1e-15 and abs(d["p"] - math.log(3.0) ** 2 / 2.0) <= 1e-15
    d = _seq(exe, [-3.5] * 7)
    assert d["lppd"] == -3.5 and d["p"] == 0.0
    d = _seq(exe, [-700.0, 0.0])                              # exp(-700) is a normal double: nothing underflows on the way
    assert abs(d["lppd"] - math.log(0.5)) <= 1e-15 and abs(d["p"] - 245000.0) <= 1e-9
    d = _seq(exe, [0.0, -700.0, -1400.0])                     # exp(-1400) underflows to 0: the maximum carries the sum
    assert abs(d["lppd"] - math.log(1.0 / 3.0)) <= 1e-15

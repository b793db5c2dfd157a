"""The erm_run planner and its executor loop (extendedrtirtmodeling.jl_amd/csrc/erm_schedule.hpp) on the CPU: the header Engine::run_checked calls is compiled
by g++ with UndefinedBehaviorSanitizer and -ftrapv into tests/schedule_check.cpp, which plans calls of 0 ... 200, 2^20 - 1 ... 2^20 + 1 and 2^31 - 1 sweeps for
every combination of model family, schedule, sharding, flags, profile mode, resident statistics and calibration an engine can produce, checks every plan against
the rules the schedule keeps (every sweep once, run-begin first, closing tiny step and run-end last and once, graphs replayed at buffer parity 0 only, at
most four replays per event bracket, no graph built inside a bracket) by running it through run_steps() on an executor of counters, and compares the
timed-sweep count with the closed form of the schedule code the planner replaced.  The named cases below are the calls the rounds tuned."""
import os
import subprocess

import pytest

import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "schedule_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sched") / "schedule_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, SRC, "-o", out], check=True)
    return out


def plan(exe, nsweeps, *, cq=0, fused=1, persist=0, shard=0, no_graph=0, profile=0, stats_valid=1, calibrate=0, gs=32):
    r = subprocess.run([exe, "case"] + [str(v) for v in (nsweeps, cq, fused, persist, shard, no_graph, profile, stats_valid, calibrate, gs)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    d = dict(kv.split("=", 1) for kv in r.stdout.split())
    return d["plan"], int(d["pass_launches"]), int(d["brackets"])


def test_sweep_has_no_undefined_behaviour_and_every_plan_keeps_the_rules(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "invariant failures 0" in r.stdout, r.stdout


def test_a_continuing_call_of_up_to_32_sweeps_is_one_graph(exe):
    """bench.py's 20-step call: run-begin, 20 sweeps, the closing tiny step and run-end replay from full[20]; in profile mode one bracket holds the call."""
    assert plan(exe, 20) == ("full:20", 0, 0)
    assert plan(exe, 20, profile=1) == ("full:20/t1", 20, 1)
    assert plan(exe, 32, profile=1) == ("full:32/t1", 32, 1)
    assert plan(exe, 1, profile=1) == ("full:1/t1", 1, 1)
    assert plan(exe, 20, cq=1, fused=0) == ("full:20", 0, 0)


def test_longer_continuing_calls_end_in_a_tail_graph(exe):
    assert plan(exe, 33, profile=1) == ("begin,block:32/t1,tail:1/t1", 33, 1)
    assert plan(exe, 64, profile=1) == ("begin,block:32/t1,tail:32/t1", 64, 1)
    assert plan(exe, 68, profile=1) == ("begin,block:32x2/t1,tail:4/t1", 68, 1)
    assert plan(exe, 88, profile=1) == ("begin,block:32x2/t1,tail:24/t1", 88, 1)
    assert plan(exe, 200, profile=1) == ("begin,block:32x6/t1,tail:8/t1", 200, 2)      # seven replays: brackets of four and three
    assert plan(exe, 88) == ("begin,block:32x2,tail:24", 0, 0)


def test_first_call_after_set_state_and_the_calibrating_call_have_no_whole_call_graph(exe):
    """Without resident statistics the prologue pass precedes the sweeps; the calibrating call (a profiling engine's first) keeps its empty event pairs
    ahead of the sweeps: block graphs largest first, then at most one single sweep, timed with them."""
    assert plan(exe, 20, stats_valid=0) == ("begin,prologue,block:16,block:4,close,end", 0, 0)
    assert plan(exe, 20, stats_valid=0, profile=1, calibrate=1) == ("begin,prologue,block:16/t1,block:4/t1,close,end", 20, 1)
    assert plan(exe, 33, stats_valid=1, profile=1, calibrate=1) == ("begin,block:32/t1,single:1/t1,close,end", 33, 2)
    assert plan(exe, 88, stats_valid=0) == ("begin,prologue,block:32x2,block:16,block:4x2,close,end", 0, 0)
    assert plan(exe, 0) == ("begin,close,end", 0, 0)
    assert plan(exe, 0, stats_valid=0, persist=1) == ("begin,prologue,close,end", 0, 0)


def test_profiled_cross_family_and_sharded_calls_time_single_sweeps(exe):
    """Their sweeps hold more than the sweep kernel, so brackets go around single kernels (two per Cross-family sweep): every sweep of a call shorter than
    68 = 2 * (32 + 2), and in longer ones a timed and an untimed sweep ahead of every block graph and every eighth sweep of the rest."""
    assert plan(exe, 20, cq=1, fused=0, profile=1) == ("begin,single:1x20/t1,close,end", 40, 40)
    assert plan(exe, 67, cq=1, fused=0, profile=1) == ("begin,single:1x67/t1,close,end", 134, 134)
    assert plan(exe, 68, cq=1, fused=0, profile=1) == ("begin,repeat:2x2,single:1x2/t2,block:32,close,end", 4, 4)
    assert plan(exe, 88, cq=1, fused=0, profile=1, stats_valid=0, calibrate=1) == ("begin,prologue,repeat:2x2,single:1x2/t2,block:32,single:1x20/t8,close,end", 10, 10)
    assert plan(exe, 88, fused=0, profile=1) == ("begin,repeat:2x2,single:1x2/t2,block:32,single:1x20/t8,close,end", 5, 5)
    assert plan(exe, 88, shard=2, stats_valid=0, profile=1) == ("begin,prologue,repeat:2x2,single:1x2/t2,block:32,single:1x20/t8,close,end", 5, 5)
    assert plan(exe, 88, shard=2, stats_valid=0) == ("begin,prologue,block:32x2,block:16,block:4x2,close,end", 0, 0)
    assert plan(exe, 88, shard=1, stats_valid=0, profile=1) == ("begin,prologue,single:1x88/t8,close,end", 11, 11)      # a callback exchange cannot be captured
    assert plan(exe, 88, no_graph=1, profile=1) == ("begin,single:1x88/t1,close,end", 88, 88)


def test_persistent_calls_are_launches_of_up_to_2_20_sweeps(exe):
    assert plan(exe, 88, persist=1, profile=1) == ("begin,persist:88/t1,close,end", 88, 1)
    assert plan(exe, 88, persist=1, stats_valid=0) == ("begin,prologue,persist:88,close,end", 0, 0)
    assert plan(exe, (1 << 20) + 1, persist=1, profile=1) == ("begin,persist:1048576/t1,persist:1/t1,close,end", (1 << 20) + 1, 2)
    assert plan(exe, 3 << 20, persist=1)[0] == "begin,persist:1048576x3,close,end"
    assert plan(exe, 10 ** 6, no_graph=1)[0] == "begin,single:1x1000000,close,end"       # a step with a count, not a million steps

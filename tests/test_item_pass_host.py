"""The plain C++ half of csrc/erm_item_pass.hpp on the CPU: the header the six item-trace passes' host path is built on, compiled by g++ with
UndefinedBehaviorSanitizer and -ftrapv into tests/item_pass_check.cpp.
  - item_pass_chunk against Python integers at the corners of its two callers: the plausible values' 20 K bytes per subject at K = 1 and K = 4096, PSIS-LOO's 8 S
    bytes at its row maximum and capped, a subject that exceeds the budget alone, a large N with a negative cap.
  - the refusals built from the table of passes against the literal strings the library has always returned."""
import os
import subprocess

import pytest

import parity_util as pu

SRC = os.path.join(pu.ROOT, "tests", "item_pass_check.cpp")
INC = os.path.join(pu.ROOT, "extendedrtirtmodeling.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("item_pass") / "item_pass_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ftrapv", "-I", INC, SRC, "-o", out], check=True)
    return out


def _run(exe, args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


CHUNKS = [(20, 1, 0),                       # plausible values, K = 1
          (20 * 4096, 10 ** 6, 0),          # plausible values, K = 4096
          (8 * 8192, 67, 1),                # PSIS at its row maximum
          (8 * 25, 300, 23),                # PSIS, capped
          (1 << 30, 5, 0),                  # one subject exceeds the budget
          (8, (1 << 32) - 1, -4)]           # large N, negative cap


def test_chunk_length_against_python_integers(exe):
    got = [int(v) for v in _run(exe, ["chunk", *(x for c in CHUNKS for x in c)])]
    want = [min(N, max(1, (256 << 20) // per), cap if cap > 0 else N) for per, N, cap in CHUNKS]
    assert got == want
    assert want == [1, 3276, 1, 23, 1, 33554432]      # worked by hand: each row takes the branch its comment names


SHARD = " not available on a shard (every subject's data must be resident on one device)"
WORDS = [  # noun, on a shard, (fewest rows of an engine, its refusal), (fewest rows of a farm chain, its refusal): the library's strings before there was a table
    ("the marginal WAIC", "the marginal WAIC is" + SHARD, (2, "the marginal WAIC needs at least two post-burn-in rows"),
     (2, "the marginal WAIC needs at least two post-burn-in rows")),
    ("the marginal LOO", "the marginal LOO is" + SHARD, (0, "-"), (1, "the marginal LOO needs post-burn-in rows (25 .. 8192 over the chains)")),
    ("the scores", "the scores are" + SHARD, (1, "the scores need at least one post-burn-in row"), (1, "the scores need at least one post-burn-in row")),
    ("the plausible values", "the plausible values are" + SHARD, (1, "the plausible values need at least one post-burn-in row"),
     (1, "the plausible values need at least one post-burn-in row")),
    ("the person fit", "the person fit is" + SHARD, (1, "the person fit needs at least one post-burn-in row"), (1, "the person fit needs at least one post-burn-in row")),
    ("the item fit", "the item fit is" + SHARD, (1, "the item fit needs at least one post-burn-in row"), (1, "the item fit needs at least one post-burn-in row")),
]


def test_refusal_words_are_the_literal_strings(exe):
    out = _run(exe, ["words"])
    assert len(WORDS) == 6 and len(out) == 4 * len(WORDS)
    for p, (noun, shard, engine, farm) in enumerate(WORDS):
        got = out[4 * p:4 * p + 4]
        assert got[0] == noun and got[1] == shard
        for line, (rows, words) in zip(got[2:], (engine, farm)):
            n, _, w = line.partition(" ")
            assert (int(n), w) == (rows, words)

"""The role-to-block-range arithmetic of the pre-pass launch (csrc/gnna_launch.h: prepass_grid, prepass_role_of), no GPU: a
small program with its own main includes the header alone, is compiled with the host C++ compiler under AddressSanitizer and
UndefinedBehaviorSanitizer, and walks every block of every grid it is given the way the kernel does.

What it asserts, for both block orders (stage range ahead of the fill range / stage and fill blocks alternating): every block of
[0, total) belongs to exactly one role, the blocks of a role carry the indices 0 .. count - 1 once each and the role's own count,
the counts add up to the grid (no overlap, no hole), the split blocks come first and the check block behind them.  The shapes: a
role without blocks (each of the four, and three at once), one block in all, passes capped at 8 blocks per compute unit, unequal
stage and fill ranges (the alternation runs out on either side), and sizes of 2^32 work items and beyond.  The block counts
themselves are pinned against the rule every launcher of a grid-stride pass carries: ceil(items / 256), at least 1, at most
8 * compute units, none for no items."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")

PROGRAM = r"""
#include "gnna_launch.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::abort(); } } while (0)

int main(int argc, char **argv)
{
    using namespace gnna;
    for (int i = 1; i + 5 < argc; i += 6) {
        const unsigned long long stage = std::strtoull(argv[i], nullptr, 10), fill = std::strtoull(argv[i + 1], nullptr, 10);
        const bool check = std::atoi(argv[i + 2]) != 0;
        const unsigned split = (unsigned)std::strtoul(argv[i + 3], nullptr, 10);
        const int cus = std::atoi(argv[i + 4]);
        const bool interleave = std::atoi(argv[i + 5]) != 0;
        const PrepassGrid g = prepass_grid(stage, fill, check, split, cus, interleave);
        unsigned long long sum = 0;
        std::vector<std::vector<unsigned char>> seen(PREPASS_ROLES);
        for (int r = 0; r < PREPASS_ROLES; r++) { seen[r].assign(g.count[r], 0); sum += g.count[r]; }
        CHECK(sum == g.total);
        int runs = 0, prev = -1;
        for (unsigned b = 0; b < g.total; b++) {
            const PrepassRole r = prepass_role_of(g, b);
            CHECK(r.role >= 0 && r.role < PREPASS_ROLES);
            CHECK(r.count == g.count[r.role] && r.index < r.count);
            CHECK(seen[r.role][r.index] == 0);
            seen[r.role][r.index] = 1;
            if (b < g.count[PREPASS_SPLIT]) CHECK(r.role == PREPASS_SPLIT && r.index == b);
            else if (b < g.count[PREPASS_SPLIT] + g.count[PREPASS_CHECK]) CHECK(r.role == PREPASS_CHECK);
            else CHECK(r.role == PREPASS_STAGE || r.role == PREPASS_FILL);
            if (r.role != prev) { runs++; prev = r.role; }
        }
        for (int r = 0; r < PREPASS_ROLES; r++)
            for (unsigned k = 0; k < g.count[r]; k++) CHECK(seen[r][k] == 1);
        std::printf("%u %u %u %u %u %d\n", g.count[PREPASS_STAGE], g.count[PREPASS_FILL], g.count[PREPASS_CHECK], g.count[PREPASS_SPLIT],
                    g.total, runs);
    }
    return 0;
}
"""

# (stage items, fill items, check, split steps, compute units) -> (stage, fill, check, split) blocks
CASES = [
    ((0, 1, 0, 0, 256), (0, 1, 0, 0)),                          # one block in all
    ((0, 4096, 1, 12, 256), (0, 16, 1, 12)),                    # no stage role (a caller's gapped layout)
    ((4096, 4096, 0, 0, 256), (16, 16, 0, 0)),                  # neither check nor split (an unprepared call)
    ((300, 70000, 1, 0, 256), (2, 274, 1, 0)),                  # the alternation runs out of stage blocks
    ((70000, 300, 1, 3, 256), (274, 2, 1, 3)),                  # ... and of fill blocks
    ((3727440, 3727440, 1, 388, 256), (2048, 2048, 1, 388)),    # the headline: both passes capped at 8 blocks per compute unit
    ((524289, 524288, 1, 5, 256), (2048, 2048, 1, 5)),          # the first size over the cap, and the last one under it
    ((524288, 524287, 0, 1, 304), (2048, 2048, 0, 1)),
    ((1 << 32, (1 << 32) + 5, 1, 512, 256), (2048, 2048, 1, 512)),
    (((1 << 40) + 255, 1 << 33, 1, 512, 8), (64, 64, 1, 512)),
    ((1, (1 << 64) - 1, 0, 0, 1), (1, 8, 0, 0)),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """One compile, one run: every grid on the command line, in both block orders."""
    d = tmp_path_factory.mktemp("prepass_grid")
    src, exe = str(d / "grid.cpp"), str(d / "grid")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, src, "-o", exe])
    asked = [k + (order,) for k, _ in CASES for order in (0, 1)]
    run = subprocess.run([exe] + [str(x) for q in asked for x in q], text=True, capture_output=True)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(asked)
    return {q: tuple(int(x) for x in line.split()) for q, line in zip(asked, out)}


@pytest.mark.parametrize("order", [0, 1], ids=["ranges", "alternating"])
@pytest.mark.parametrize("args, want", CASES, ids=["case%d" % i for i in range(len(CASES))])
def test_ranges_tile_the_grid(answers, args, want, order):
    got = answers[args + (order,)]
    assert got[:4] == want and got[4] == sum(want)


@pytest.mark.parametrize("args, runs", [((300, 70000, 1, 0, 256), {0: 3, 1: 5}), ((70000, 300, 1, 3, 256), {0: 4, 1: 7}),
                                        ((0, 4096, 1, 12, 256), {0: 3, 1: 3})])
def test_runs_of_roles(answers, args, runs):
    """Stage ahead of fill: one run per role that has blocks.  Alternating: 2 * min(stage, fill) runs of one block, then what is
    left of the longer range (which continues the last run when that is the fill range)."""
    for order, want in runs.items():
        assert answers[args + (order,)][5] == want

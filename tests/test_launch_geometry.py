"""Launch geometry of the gather kernels, pinned (no GPU): a small program with its own main includes csrc/gnna_launch.h alone,
is compiled with the host C++ compiler (g++, as oracle/ compiles its sources) and prints what chunk_grid, log2_lanes and
attn_layout answer.
The expected values were worked out by hand from the formula every launcher carried before it was shared: G = max(1, min(64,
2048 / partSize)), halved while ceil(P / G) < 16 * num_cus; blocks = ceil(ceil(P / G) / 4).  A slip here costs speed, not
correctness, so no parity test would see it.  attn_layout is the lane layout of the fused attention kernels: log_lph =
log2_lanes(dim, 4), then log_lpr raised from log_lph while log_lpr < 6 and 2^(log_lpr - log_lph) < heads; the values were worked
out by hand from that rule.  The shape table of tests/attn_cases.py (what the GPU tests of the attention kernels run) is put to
the same program: its base set must hit each of the 28 layouts exactly once and its column-block set must need more than one
wave-wide load per row, by the header's own answer."""
import os
import subprocess

import pytest

import attn_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnnadvisor_osdi21_amd", "csrc")

# (num_parts, partSize, num_cus) -> (G, blocks)
CHUNK_GRID = [
    ((1, 32, 256), (1, 1)),
    ((5000, 32, 256), (1, 1250)),
    ((10000, 32, 256), (2, 1250)),
    ((262145, 32, 256), (64, 1025)),
    ((262080, 32, 256), (32, 2048)),
    ((81923, 100, 256), (20, 1025)),
    ((81900, 100, 256), (10, 2048)),
    ((257, 4096, 256), (1, 65)),
    ((1000, 32, 1), (64, 4)),
]
LANES_4 = dict(zip((1, 4, 5, 8, 9, 64, 65, 128, 129, 256, 257, 1000), (0, 0, 1, 1, 2, 4, 5, 5, 6, 6, 6, 6)))
LANES_8 = dict(zip((8, 9, 512, 513), (0, 1, 6, 6)))
# (heads, dim) -> (log_lph, log_lpr); the first eight are the shapes the GPU tests of the three attention families run (8 x 40:
# capped, 4 heads per column block, so two blocks)
ATTN_LAYOUT = [
    ((1, 64), (4, 4)),
    ((4, 16), (2, 4)),
    ((3, 5), (1, 3)),
    ((8, 8), (1, 4)),
    ((1, 256), (6, 6)),
    ((64, 1), (0, 6)),
    ((2, 33), (4, 5)),
    ((8, 40), (4, 6)),
    ((1, 1), (0, 0)),
    ((1, 4), (0, 0)),
    ((1, 5), (1, 1)),
    ((2, 4), (0, 1)),
]

PROGRAM = r"""
#include "gnna_launch.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int i = 1; i + 3 < argc; i += 4) {
        const long long a = std::atoll(argv[i + 1]);
        const int b = std::atoi(argv[i + 2]), c = std::atoi(argv[i + 3]);
        if (argv[i][0] == 'g') {
            const gnna::ChunkGrid g = gnna::chunk_grid(a, b, c);
            std::printf("%d %lld\n", g.G, (long long)g.blocks);
        } else if (argv[i][0] == 'a') {
            const gnna::AttnLayout y = gnna::attn_layout((int)a, b);
            std::printf("%d %d\n", y.log_lph, y.log_lpr);
        } else {
            std::printf("%d\n", gnna::log2_lanes((int)a, b));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """One compile, one run: every question on the command line, one answer per line."""
    d = tmp_path_factory.mktemp("launch_geometry")
    src, exe = str(d / "geometry.cpp"), str(d / "geometry")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, src,
                           "-o", exe])
    asked = [("g",) + k for k, _ in CHUNK_GRID] + [("l", d_, 4, 0) for d_ in LANES_4] + [("l", d_, 8, 0) for d_ in LANES_8]
    asked += [("a",) + k + (0,) for k, _ in ATTN_LAYOUT]
    asked += [("a",) + k + (0,) for k in attn_cases.ALL_SHAPES if ("a",) + k + (0,) not in asked]
    out = subprocess.check_output([exe] + [str(x) for q in asked for x in q], text=True).splitlines()
    assert len(out) == len(asked)
    return {q: tuple(int(x) for x in line.split()) for q, line in zip(asked, out)}


@pytest.mark.parametrize("args, want", CHUNK_GRID, ids=["P%d_ps%d_cus%d" % k for k, _ in CHUNK_GRID])
def test_chunk_grid(answers, args, want):
    assert answers[("g",) + args] == want


def test_log2_lanes(answers):
    assert {d: answers[("l", d, 4, 0)][0] for d in LANES_4} == LANES_4
    assert {d: answers[("l", d, 8, 0)][0] for d in LANES_8} == LANES_8


@pytest.mark.parametrize("args, want", ATTN_LAYOUT, ids=["%dx%d" % k for k, _ in ATTN_LAYOUT])
def test_attn_layout(answers, args, want):
    assert answers[("a",) + args + (0,)] == want


def test_the_shape_table_hits_each_of_the_28_layouts_once(answers):
    got = [answers[("a",) + k + (0,)] for k in attn_cases.BASE_SHAPES]
    every = [(lph, lpr) for lph in range(7) for lpr in range(lph, 7)]
    assert len(every) == 28 and sorted(got) == every, sorted(set(every) - set(got))
    for lph, shapes in attn_cases.BASE.items():                       # and the table files each shape under its own log_lph
        assert [answers[("a",) + k + (0,)] for k in shapes] == [(lph, lpr) for lpr in range(lph, 7)], lph
    assert all(h <= 64 and d <= 256 for h, d in attn_cases.ALL_SHAPES)  # (what the entries accept)


def test_the_column_block_shapes_need_several_blocks(answers):
    """One per log_lph = 1 .. 6: log_lpr = 6 and more heads than the 2^(6 - log_lph) a wave-wide load holds; the first five end
    in a partial block (log_lph = 0 has no such shape: 64 heads of at most 4 floats fit one load, and 64 heads is the most)."""
    assert len(attn_cases.COLUMN_BLOCKS) == 6
    for k, (heads, dim) in enumerate(attn_cases.COLUMN_BLOCKS):
        log_lph, log_lpr = answers[("a", heads, dim, 0)]
        per_block = 1 << (log_lpr - log_lph)
        assert (log_lph, log_lpr) == (k + 1, 6) and heads > per_block, (heads, dim)
        assert (heads % per_block != 0) == (k < 5), (heads, dim)

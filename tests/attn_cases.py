"""The shapes and launch geometries the tests of the fused attention kernels share (checker side only; nothing here reads the
library, so the host tests use it without a GPU).

Shapes.  attn_layout(heads, dim) of csrc/gnna_launch.h picks (log_lph, log_lpr) with 0 <= log_lph <= log_lpr <= 6: 28 layouts,
each a template instance of every pull kernel and of the shared lse pass with its own folds.  BASE holds one (heads, dim) per
layout -- about half of the head counts are no power of two (some head slots of a row idle), most dims no multiple of 4 (a
partial last piece).  COLUMN_BLOCKS holds one shape per log_lph = 1 .. 6 with more heads than one wave-wide load holds
(heads > 64 / LPH, log_lpr = 6), so the column-block loop runs; the first five end in a partial block.  The widest row is 390
floats.  tests/test_launch_geometry.py proves both claims against the compiled header.

Geometries.  chunk_grid(P, partSize, CUs) halves G while there are fewer than T = 16 * CUs chunks, so only a structure of several
T neighbor-groups gives a wavefront more than one group: GEOMETRIES are (name, P from T, partSize, G) for
gat_rect_ref.multi_run_structure."""
import numpy as np

# log_lph -> (heads, dim); log_lpr = log_lph .. 6 in this order
BASE = {
    0: [(1, 3), (2, 4), (3, 1), (8, 2), (9, 3), (32, 4), (33, 3)],
    1: [(1, 7), (2, 5), (3, 8), (8, 6), (16, 5), (17, 7)],
    2: [(1, 13), (2, 16), (3, 9), (8, 12), (9, 10)],
    3: [(1, 17), (2, 32), (3, 29), (5, 24)],
    4: [(1, 33), (2, 64), (3, 50)],
    5: [(1, 65), (2, 128)],
    6: [(1, 129)],
}
COLUMN_BLOCKS = [(33, 5), (17, 9), (9, 20), (5, 64), (3, 100), (3, 130)]       # log_lph = 1 .. 6
BASE_SHAPES = [s for lph in sorted(BASE) for s in BASE[lph]]
ALL_SHAPES = BASE_SHAPES + COLUMN_BLOCKS
assert len(BASE_SHAPES) == 28 and len(set(ALL_SHAPES)) == 34 and max(h * d for h, d in ALL_SHAPES) <= 512

# (id, num_parts from T = 16 * compute units, partSize, G): 64 T + 1 leaves one group in the last chunk; 5 is no power of two
GEOMETRIES = [("64T+1_ps1", lambda T: 64 * T + 1, 1, 64), ("2T+5_ps1", lambda T: 2 * T + 5, 1, 2), ("7T_ps100", lambda T: 7 * T, 100, 5)]
CHUNK_SHAPES = [(1, 64), (4, 16), (3, 5), (2, 33)]
WAVES_PER_BLOCK = 4


def chunk_grid(num_parts, partSize, num_cus):
    """(G, blocks) of gnna::chunk_grid, restated (the header's own answers are pinned in tests/test_launch_geometry.py)."""
    G = max(1, min(64, 2048 // max(1, partSize)))
    while G > 1 and -(-num_parts // G) < num_cus * 16:
        G >>= 1
    chunks = -(-num_parts // G)
    return G, -(-chunks // WAVES_PER_BLOCK)


def runs_of(p2n, G):
    """What the wavefronts make of the groups p2n [P] at G groups per chunk: a run is a maximal stretch of consecutive groups of
    one row inside one chunk.  -> dict(runs_per_chunk [chunks], groups_per_run [runs], rows_cut_by_chunk, rows_cut_by_block):
    the numbers of rows whose groups lie in more than one chunk / workgroup (4 chunks)."""
    p2n = np.asarray(p2n, dtype=np.int64)
    P = len(p2n)
    chunk = np.arange(P) // G
    first = np.ones(P, dtype=bool)
    first[1:] = (p2n[1:] != p2n[:-1]) | (chunk[1:] != chunk[:-1])
    run_id = np.cumsum(first) - 1
    same_row = p2n[1:] == p2n[:-1]
    return dict(runs_per_chunk=np.bincount(chunk[first], minlength=chunk[-1] + 1), groups_per_run=np.bincount(run_id),
                rows_cut_by_chunk=len(np.unique(p2n[1:][same_row & (chunk[1:] != chunk[:-1])])),
                rows_cut_by_block=len(np.unique(p2n[1:][same_row & (chunk[1:] // WAVES_PER_BLOCK != chunk[:-1] // WAVES_PER_BLOCK)])))

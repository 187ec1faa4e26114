"""not-gpu: the block -> tile map of the second bottleneck64 kernel (occ_bottleneck64_tile_of_block, a pure function) is a
permutation of the tiles for every grid, blocks that share an XCD (b, b + 8, ...) walk neighbouring tiles, and the forced-
variant entry point checks its arguments before any launch."""
import ctypes

import pytest

from occnet_amd import _lib

BAND = 4     # tile rows per band of order 2 (csrc/bottleneck64_v2_nhwc_bf16.hip: kBnBand)

GRIDS = sorted({(b, ty, tx) for b in (1, 2, 3) for ty in range(1, 7) for tx in range(1, 7)}) + [(6, 29, 25)]


def _walk(batch, tiles_y, tiles_x, order):
    """The order's walk over the tiles, written down independently of the C code: a list of row-major tile indices."""
    tiles = []
    for img in range(batch):
        if order == 1:
            tiles += [(img, ty, tx) for ty in range(tiles_y) for tx in range(tiles_x)]
        else:
            for r0 in range(0, tiles_y, BAND):
                rows = range(r0, min(r0 + BAND, tiles_y))
                tiles += [(img, ty, tx) for tx in range(tiles_x) for ty in rows]
    return [(img * tiles_y + ty) * tiles_x + tx for img, ty, tx in tiles]


def _map(n, tiles_x, tiles_y, order):
    f = _lib.lib().occ_bottleneck64_tile_of_block
    return [f(b, n, tiles_x, tiles_y, order) for b in range(n)]


def test_grids_cover_the_small_and_ragged_block_counts():
    counts = {b * ty * tx for b, ty, tx in GRIDS}
    assert {1, 2, 3, 4, 5, 6}.issubset(counts)                            # fewer blocks than XCDs
    assert {8, 16, 24, 9, 12, 27, 50, 75, 108}.issubset(counts)           # whole rounds of 8, and every kind of remainder
    assert {n % 8 for n in counts} == set(range(8)) and 6 * 29 * 25 in counts


@pytest.mark.parametrize("order", [0, 1, 2])
def test_map_is_a_permutation_of_the_tiles(order):
    for batch, tiles_y, tiles_x in GRIDS:
        n = batch * tiles_y * tiles_x
        got = _map(n, tiles_x, tiles_y, order)
        assert sorted(got) == list(range(n)), (batch, tiles_y, tiles_x)
        if order == 0:
            assert got == list(range(n))


@pytest.mark.parametrize("order", [1, 2])
def test_blocks_of_one_xcd_walk_neighbouring_tiles(order):
    for batch, tiles_y, tiles_x in GRIDS:
        n = batch * tiles_y * tiles_x
        got = _map(n, tiles_x, tiles_y, order)
        walk = _walk(batch, tiles_y, tiles_x, order)
        pos = {t: i for i, t in enumerate(walk)}
        q, r = divmod(n, 8)
        for b in range(n):
            x = b % 8
            # group x owns the contiguous range of the walk that starts at x*q + min(x, r) ...
            assert pos[got[b]] == x * q + min(x, r) + b // 8, (batch, tiles_y, tiles_x, b)
            # ... so b and b + 8 compute tiles that follow each other in it
            if b + 8 < n:
                assert pos[got[b + 8]] == pos[got[b]] + 1
        # and tiles that follow each other in the walk touch, unless a row, band or image ends between them
        per_img = tiles_y * tiles_x
        for a, c in zip(walk, walk[1:]):
            (ia, ra), (ic, rc) = divmod(a, per_img), divmod(c, per_img)
            (ya, xa), (yc, xc) = divmod(ra, tiles_x), divmod(rc, tiles_x)
            if order == 1:
                assert (ia == ic and ya == yc and xc == xa + 1) or xc == 0
            else:
                assert (ia == ic and xa == xc and yc == ya + 1) or yc % BAND == 0


def test_map_entry_rejects_bad_arguments():
    f = _lib.lib().occ_bottleneck64_tile_of_block
    assert f(0, 12, 3, 2, 1) >= 0
    assert f(12, 12, 3, 2, 1) == -1 and f(-1, 12, 3, 2, 1) == -1          # block outside the grid
    assert f(0, 13, 3, 2, 1) == -1 and f(0, 0, 3, 2, 1) == -1             # not whole images of tiles
    assert f(0, 12, 0, 2, 1) == -1 and f(0, 12, 3, 0, 1) == -1
    assert f(0, 12, 3, 2, 3) == -1 and f(0, 12, 3, 2, -1) == -1           # no such order
    assert b'bottleneck64_tile_of_block' in _lib.lib().occ_last_error()


def test_variant_entry_point_checks_arguments_without_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.cast(buf, ctypes.c_void_p), None
    f = lib.occ_bottleneck64_nhwc_bf16_variant
    for v in (0, 1, 2, 3, 4, 5):
        for i in range(8):                                                # each of the eight pointers
            a = [p] * 8
            a[i] = null
            assert f(*a, 1, 4, 4, 256, 0, v, null) == -1
        assert b'null pointer' in lib.occ_last_error()
        assert f(*[p] * 8, 0, 4, 4, 256, 0, v, null) == -1                # batch 0
        assert f(*[p] * 8, 1, 4, 4, 128, 0, v, null) == -3                # Cin 128
        assert f(*[p] * 8, 1, 4, 4, 64, 0, v, null) == -3                 # Cin 64 needs the projection
        assert b'no kernel' in lib.occ_last_error()
    for v in (6, 7, 22, 100, -1, -2):
        assert f(*[p] * 8, 1, 4, 4, 256, 0, v, null) == -3                # unknown variant, refused before any launch
        assert b'no variant' in lib.occ_last_error()
        assert f(*[p] * 8, 1, 4, 4, 64, 1, v, null) == -3

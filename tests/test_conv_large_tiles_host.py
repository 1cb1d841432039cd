"""Host side of the pixel-heavy tiles of csrc/conv_large.hip: the tile `conv3x3_large` runs a class on is what the committed
sweep (profiles/r17_conv_large_tiles_sweep.log, tools/conv_large_sweep.py) shows faster than the shape rule's tile in both
directions by more than the spread of the replays, and the shape rule's tile for everything else.  No device is needed."""
import os
import re

from diffusion_finetuning_amd import _native as nat

F16, BF16, F32 = 1, 2, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (32, 320, 352, 640, 960, 1280, 1920, 2560)
SIDE = {4096: 32, 16384: 64}


def _sweep_rows():
    """(pixels, C_in, C_out, tile) of every row, the tile recomputed from the row's own times and spreads."""
    rows = []
    num = r"\s+(\d+\.\d|nan)"
    pat = re.compile(r"\s+4\s+\d+x\d+\s+(\d+)\s+(\d+)\s+(\d+) \|" + num * 6 + r" \|" + num * 6 + r" \|\s+(yes|no)\s+\w+\s+\|\s+(\d)\s")
    for line in open(os.path.join(ROOT, "profiles", "r17_conv_large_tiles_sweep.log")):
        m = pat.match(line)
        if not m:
            continue
        pixels, cin, cout = (int(m.group(i)) for i in (1, 2, 3))
        f = [float(m.group(i)) for i in range(4, 10)]    # stock, small, large, t256, t128, spread
        b = [float(m.group(i)) for i in range(10, 16)]
        better = [t for t in (1, 2) if f[2] - f[2 + t] > f[5] and b[2] - b[2 + t] > b[5]]
        tile = min(better, key=lambda t: f[2 + t] + b[2 + t]) if better else 0
        assert tile == int(m.group(17)), line  # the log's own last column follows the same rule
        rows.append((pixels, cin, cout, tile))
    return rows


def test_the_measured_table_is_the_sweeps_tile_column_and_nothing_else():
    rows = _sweep_rows()
    assert len(rows) == 10 and {r[0] for r in rows} == {4096, 16384}
    assert any(r[3] == 1 for r in rows) and any(r[3] == 2 for r in rows)
    table = {}
    for pixels, cin, cout, tile in rows:
        table[(pixels, cin, cout)] = table[(pixels, cout, cin)] = tile
    lib = nat.lib()
    for dtype in (F16, BF16):
        for pixels, side in SIDE.items():
            for cin in CHANNELS:
                for cout in CHANNELS:
                    want = table.get((pixels, cin, cout), 0)
                    assert lib.conv3x3_large_tile_choice(4, cin, cout, side, side, dtype) == want, (pixels, cin, cout)
    for (pixels, cin, cout), tile in table.items():  # a routed class is one the planner sends to this family
        if tile:
            assert lib.conv3x3_large_plan(pixels, cin, cout, F16) == 1


def test_every_other_geometry_keeps_the_shape_rules_tile():
    lib = nat.lib()
    # the same pixel counts in other geometries, other batches of the measured sides, and the shapes of the GPU tests
    for shape in ((16, 640, 640, 16, 16), (1, 640, 640, 64, 64), (2, 320, 320, 128, 64), (8, 640, 640, 32, 32), (1, 320, 320, 64, 64),
                  (4, 32, 192, 64, 64), (4, 192, 32, 64, 64), (1, 1920, 160, 4, 64), (3, 96, 160, 3, 5), (1, 64, 96, 32, 8)):
        assert lib.conv3x3_large_supported(*shape, F16) == 1
        assert lib.conv3x3_large_tile_choice(*shape, F16) == 0, shape
    assert lib.conv3x3_large_tile_choice(4, 640, 640, 32, 32, F32) == -1
    assert lib.conv3x3_large_tile_choice(4, 48, 640, 32, 32, F16) == -1
    for shape in ((4, 640, 640, 32, 32), (4, 320, 320, 64, 64), (4, 1280, 1280, 32, 32)):
        assert lib.conv3x3_large_workspace_bytes(*shape, F16) == 0


def test_the_named_tile_entry_checks_its_arguments_without_a_gpu():
    lib = nat.lib()
    one = 16  # a non-null, 16-byte aligned "pointer"; nothing is dereferenced before the checks are through
    args = (one, one, None, one, None, 0)
    assert lib.conv3x3_large_tile(*args, 1, 32, 96, 32, 8, F16, 3, None) == -1     # unknown tiles
    assert lib.conv3x3_large_tile(*args, 1, 32, 96, 32, 8, F16, -1, None) == -1
    assert lib.conv3x3_large_tile(None, one, None, one, None, 0, 1, 32, 96, 32, 8, F16, 1, None) == -1
    assert lib.conv3x3_large_tile(*args, 1, 32, 96, 32, 8, F32, 1, None) == -5
    for shape, tile in (((1, 32, 96, 64, 6), 1), ((1, 32, 96, 64, 6), 2),          # W no multiple of 8
                        ((1, 32, 96, 20, 8), 2), ((1, 32, 96, 48, 8), 1),          # H·W no multiple of the tile
                        ((2, 32, 96, 24, 8), 2),                                   # a tile would straddle two images
                        ((1, 32, 96, 8, 24), 2),                                   # a tile is no whole number of rows
                        ((1, 32, 96, 2, 128), 2)):                                 # a row is more than half a tile
        assert lib.conv3x3_large_tile(*args, *shape, F16, tile, None) == -5, (shape, tile)
    assert lib.conv3x3_large_tile(one + 2, one, None, one, None, 0, 1, 32, 96, 32, 8, F16, 1, None) == -3

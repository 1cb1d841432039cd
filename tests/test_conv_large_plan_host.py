"""Host side of the many-pixel packed-weight 3×3 convolution (csrc/conv_large.hip): its planner, its shape envelope and its
argument checks run without a device; the small family's planner is unchanged."""
import os
import re

import torch

from diffusion_finetuning_amd import _native as nat

F16, BF16, F32 = 1, 2, 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PIXELS = (1, 256, 1024, 2304, 4095, 4096, 4097, 8192, 9216, 16384, 32768)
CHANNELS = (32, 320, 352, 640, 960, 1280, 1920, 2560)
# what conv3x3_small_plan routes (profiles/r14_conv_small_sweep.log, pinned by tests/test_conv_plan_host.py)
SMALL_ROUTED = [
    (256, 1280, 1280), (256, 2560, 1280),
    (1024, 640, 1280), (1024, 1280, 1280), (1024, 2560, 1280), (1024, 1920, 1280),
]


def _sweep_rows():
    """(pixels, C_in, C_out, wins) of every row of the committed sweep of tools/conv_large_sweep.py."""
    rows = []
    for line in open(os.path.join(ROOT, "profiles", "r15_conv_large_sweep.log")):
        m = re.match(r"\s+\d+\s+\d+x\d+\s+(\d+)\s+(\d+)\s+(\d+) \|.*\|.*\|\s+(yes|no)\s", line)
        if m:
            rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)))
    return rows


def test_the_plan_is_a_function_of_its_arguments_and_symmetric_under_the_channel_swap():
    lib = nat.lib()
    for dtype in (F16, BF16):
        for pixels in PIXELS:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    first = lib.conv3x3_large_plan(pixels, cin, cout, dtype)
                    assert first in (0, 1)
                    assert all(lib.conv3x3_large_plan(pixels, cin, cout, dtype) == first for _ in range(3))
                    assert lib.conv3x3_large_plan(pixels, cout, cin, dtype) == first  # the backward-data class


def test_the_plan_routes_the_rows_the_sweep_marks_yes_and_nothing_else():
    rows = _sweep_rows()
    assert len(rows) >= 10 and {r[0] for r in rows} <= {4096, 16384}  # the ten headline classes were measured
    wins = [r[:3] for r in rows if r[3] == "yes"]
    routed = set(wins) | {(p, co, ci) for p, ci, co in wins}
    lib = nat.lib()
    for dtype in (F16, BF16):
        for pixels in PIXELS:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    assert lib.conv3x3_large_plan(pixels, cin, cout, dtype) == int((pixels, cin, cout) in routed), (pixels, cin, cout)
        for cin in CHANNELS:
            for cout in CHANNELS:
                some = any((p, cin, cout) in routed for p in PIXELS)
                assert lib.conv3x3_large_plan_channels(cin, cout, dtype) == int(some), (cin, cout)
        for pixels, cin, cout in wins:  # every routed class is one the kernel covers, in both directions
            side = {4096: 32, 16384: 64}[pixels]
            assert lib.conv3x3_large_supported(4, cin, cout, side, side, dtype) == 1
            assert lib.conv3x3_large_supported(4, cout, cin, side, side, dtype) == 1
    for pixels, cin, cout in wins:  # the two planners never claim the same class
        assert lib.conv3x3_small_plan(pixels, cin, cout, F16) == 0


def test_the_plan_routes_nothing_for_f32_or_an_unknown_dtype():
    lib = nat.lib()
    for dtype in (F32, 7, -1):
        for pixels in PIXELS:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    assert lib.conv3x3_large_plan(pixels, cin, cout, dtype) == 0
                    assert lib.conv3x3_large_plan_channels(cin, cout, dtype) == 0
    assert lib.conv3x3_large_plan(0, 640, 640, F16) == 0 and lib.conv3x3_large_plan(-4096, 640, 640, F16) == 0
    assert not nat.conv3x3_large_plan(4096, 640, 640, torch.float32)


def test_the_small_familys_plan_is_what_it_was():
    lib = nat.lib()
    routed = set(SMALL_ROUTED) | {(p, co, ci) for p, ci, co in SMALL_ROUTED}
    for dtype in (F16, BF16):
        for pixels in PIXELS:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    assert lib.conv3x3_small_plan(pixels, cin, cout, dtype) == int((pixels, cin, cout) in routed), (pixels, cin, cout)


def test_envelope_and_workspace_refuse_the_bad_shapes_and_agree_on_the_good_ones():
    lib = nat.lib()
    for bad in ((4, 1280, 1280, 8, 8, F32), (4, 1280, 1280, 8, 8, 9), (0, 64, 64, 8, 8, F16), (4, 48, 64, 8, 8, F16),
                (4, 64, 40, 8, 8, F16), (4, 64, 64, 0, 8, F16), (4, 64, 64, 8, -1, F16), (4, 0, 64, 8, 8, F16),
                (1, 32, 32, 4, 2000, F16),           # a row with its halo does not fit a tile's staging area (384 positions)
                (64, 2560, 32, 128, 128, F16)):      # 2^31 elements of x
        assert lib.conv3x3_large_supported(*bad) == 0, bad
        assert lib.conv3x3_large_workspace_bytes(*bad) == 0, bad
    for good in ((1, 32, 32, 1, 1, F16), (3, 96, 160, 3, 5, BF16), (4, 320, 320, 64, 64, F16), (4, 1920, 640, 32, 32, F16),
                 (3, 32, 352, 2, 66, BF16), (8, 320, 320, 64, 64, F16)):
        assert lib.conv3x3_large_supported(*good) == 1, good
        assert lib.conv3x3_large_workspace_bytes(*good) == 0, good  # no split along K: no workspace


def test_argument_validation_needs_no_gpu():
    lib = nat.lib()
    one = 16  # a non-null, 16-byte aligned "pointer"; nothing is dereferenced before the checks are through
    # null pointers, non-positive sizes, unknown dtype, a negative workspace size
    assert lib.conv3x3_large(None, one, None, one, None, 0, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_large(one, None, None, one, None, 0, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_large(one, one, None, None, None, 0, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_large(one, one, None, one, None, 0, 0, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_large(one, one, None, one, None, 0, 2, 64, 64, 8, 8, 7, None) == -1
    assert lib.conv3x3_large(one, one, None, one, one, -1, 2, 64, 64, 8, 8, F16, None) == -1
    # fp32 and uncovered shapes
    assert lib.conv3x3_large(one, one, None, one, None, 0, 2, 64, 64, 8, 8, F32, None) == -5
    assert lib.conv3x3_large(one, one, None, one, None, 0, 2, 48, 64, 8, 8, F16, None) == -5
    # alignment: x, y, and a workspace that is passed although none is needed
    assert lib.conv3x3_large(one + 2, one, None, one, None, 0, 2, 64, 64, 8, 8, F16, None) == -3
    assert lib.conv3x3_large(one, one, None, one + 8, None, 0, 2, 64, 64, 8, 8, F16, None) == -3
    assert lib.conv3x3_large(one, one + 4, None, one, None, 0, 2, 64, 64, 8, 8, F16, None) == -3
    assert lib.conv3x3_large(one, one, None, one, one + 4, 64, 2, 64, 64, 8, 8, F16, None) == -3
    # the pack both families read
    assert lib.conv3x3_small_pack(None, one, 64, 64, 0, F16, None) == -1
    assert lib.conv3x3_small_pack(one, one, 64, 64, 2, F16, None) == -1
    assert lib.conv3x3_small_pack(one, one, 64, 64, 0, F32, None) == -5
    assert lib.conv3x3_small_pack(one, one, 64, 40, 1, F16, None) == -5
    assert lib.conv3x3_small_pack(one, one + 4, 64, 64, 0, F16, None) == -3


def test_the_front_keeps_cpu_calls_on_the_stock_line_and_the_forced_route_refuses_them():
    from diffusion_finetuning_amd import conv

    assert "large" in conv.ROUTES
    x, w, b = torch.randn(1, 32, 4, 4), torch.randn(32, 32, 3, 3), torch.randn(32)
    ref = torch.nn.functional.conv2d(x, w, b, padding=1)
    assert torch.equal(conv.conv3x3(x, w, b), ref) and torch.equal(conv.conv3x3(x, w, b, route="auto"), ref)
    try:
        conv.conv3x3(x, w, b, route="large")
        raise AssertionError("a CPU call must not be accepted by the forced route")
    except RuntimeError:
        pass
    layer = torch.nn.Conv2d(640, 640, 3, padding=1).requires_grad_(False)
    assert conv.prepack_conv3x3(layer) == 0 and conv.prepack_conv3x3(layer, route="large") == 0  # nothing on a device

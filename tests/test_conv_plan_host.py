"""Host side of the packed-weight 3×3 convolution (csrc/conv_small.hip): the planner, the shape envelope and the argument checks
run without a device."""
import torch

from diffusion_finetuning_amd import _native as nat

F16, BF16, F32 = 1, 2, 0

# (pixels, C_in, C_out) of the benchmark's frozen 3×3 stride-1 convolutions that the planner routes (batch 4 at 64² latents):
# the 8×8 and 16×16 levels of the SD1.5 UNet.  This list is the contract of tools/conv_small_sweep.py: a class is here only
# if the HIP kernel won there in both directions.
ROUTED = [
    (256, 1280, 1280), (256, 2560, 1280),
    (1024, 640, 1280), (1024, 1280, 1280), (1024, 2560, 1280), (1024, 1920, 1280),
]
# ... and what stays on the stock convolution: the 32² and 64² levels
STOCK = [
    (4096, 320, 640), (4096, 640, 640), (4096, 1920, 640), (4096, 1280, 640), (4096, 960, 640), (4096, 1280, 1280),
    (16384, 320, 320), (16384, 960, 320), (16384, 640, 320), (16384, 640, 640),
]


def test_the_plan_is_a_function_of_its_arguments():
    lib = nat.lib()
    for dtype in (F16, BF16):
        for pixels in (1, 64, 256, 1024, 1025, 4096, 16384):
            for cin in (32, 320, 640, 1280, 1920, 2560):
                for cout in (32, 320, 640, 1280):
                    first = lib.conv3x3_small_plan(pixels, cin, cout, dtype)
                    assert first in (0, 1)
                    assert all(lib.conv3x3_small_plan(pixels, cin, cout, dtype) == first for _ in range(3))
                    # the backward-data call is the same class with the channel roles swapped
                    assert lib.conv3x3_small_plan(pixels, cout, cin, dtype) == first


def test_the_plan_routes_the_sweeps_classes_and_nothing_else():
    """profiles/r14_conv_small_sweep.log has six rows, all at batch 4: the planner routes those classes (and their backward
    forms) at those pixel counts and no other pixel count or channel pair — not the 512 pixels of batch 8, not the 144 and 576
    of 96² latents, which nobody measured."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for line in open(os.path.join(root, "profiles", "r14_conv_small_sweep.log")):
        m = re.match(r"\s+\d+\s+\d+x\d+\s+(\d+)\s+(\d+)\s+(\d+) \|.*\|\s+(yes|no)\s", line)
        if m:
            rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)))
    assert sorted(r[:3] for r in rows if r[3] == "yes") == sorted(ROUTED) and all(r[3] == "yes" for r in rows)
    lib = nat.lib()
    routed = set(ROUTED) | {(p, co, ci) for p, ci, co in ROUTED}
    channels = (32, 320, 640, 672, 960, 1248, 1280, 1312, 1600, 1920, 2240, 2560, 2592)
    for dtype in (F16, BF16):
        for pixels in (1, 16, 64, 128, 144, 255, 256, 257, 512, 576, 1023, 1024, 1025, 2048, 2304, 4096, 16384):
            for cin in channels:
                for cout in channels:
                    assert lib.conv3x3_small_plan(pixels, cin, cout, dtype) == int((pixels, cin, cout) in routed), (pixels, cin, cout)
        for cin in channels:
            for cout in channels:
                some = any((p, cin, cout) in routed for p in (256, 1024))
                assert lib.conv3x3_small_plan_channels(cin, cout, dtype) == int(some), (cin, cout)
        for pixels, cin, cout in ROUTED:
            side = 8 if pixels == 256 else 16
            assert lib.conv3x3_small_supported(4, cin, cout, side, side, dtype) == 1
            assert lib.conv3x3_small_supported(4, cout, cin, side, side, dtype) == 1
        for pixels, cin, cout in STOCK:
            assert lib.conv3x3_small_plan(pixels, cin, cout, dtype) == 0, (pixels, cin, cout)
    assert lib.conv3x3_small_plan_channels(1280, 1280, F32) == 0 and lib.conv3x3_small_plan_channels(1280, 1280, 7) == 0
    assert nat.conv3x3_small_plan_channels(1280, 640, torch.float16) and not nat.conv3x3_small_plan_channels(1920, 640, torch.float16)


def test_plan_and_envelope_refuse_what_the_kernel_does_not_cover():
    lib = nat.lib()
    assert lib.conv3x3_small_plan(256, 1280, 1280, F32) == 0 and lib.conv3x3_small_plan(256, 1280, 1280, 7) == 0
    assert lib.conv3x3_small_plan(0, 1280, 1280, F16) == 0 and lib.conv3x3_small_plan(-5, 1280, 1280, F16) == 0
    assert lib.conv3x3_small_plan(256, 1290, 1280, F16) == 0 and lib.conv3x3_small_plan(256, 1280, 1296, F16) == 0
    for bad in ((4, 1280, 1280, 8, 8, F32), (4, 1280, 1280, 8, 8, 9), (0, 64, 64, 8, 8, F16), (4, 48, 64, 8, 8, F16),
                (4, 64, 40, 8, 8, F16), (4, 64, 64, 0, 8, F16), (4, 64, 64, 8, -1, F16), (4, 0, 64, 8, 8, F16),
                (1, 32, 32, 4, 2000, F16),           # a row with its halo does not fit a tile's staging area (768 positions)
                (64, 2560, 32, 128, 128, F16)):      # 2^31 elements of x
        assert lib.conv3x3_small_supported(*bad) == 0, bad
        assert lib.conv3x3_small_workspace_bytes(*bad) == 0, bad
    for good in ((1, 32, 32, 1, 1, F16), (3, 96, 160, 3, 5, BF16), (4, 2560, 1280, 8, 8, F16), (1, 1280, 1280, 24, 24, F16),
                 (8, 320, 320, 64, 64, F16)):
        assert lib.conv3x3_small_supported(*good) == 1, good
        ws = lib.conv3x3_small_workspace_bytes(*good)
        assert ws > 0 and ws % 16 == 0 and ws == lib.conv3x3_small_workspace_bytes(*good)
        N, cin, cout, H, W, _ = good
        assert ws >= N * H * W * cout * 4  # at least one fp32 partial per output element


def test_argument_validation_needs_no_gpu():
    lib = nat.lib()
    one = 16  # a non-null, 16-byte aligned "pointer"; nothing is dereferenced before the checks are through
    ws = lib.conv3x3_small_workspace_bytes(2, 64, 64, 8, 8, F16)
    # null pointers, non-positive sizes, unknown dtype
    assert lib.conv3x3_small(None, one, None, one, one, ws, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_small(one, None, None, one, one, ws, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_small(one, one, None, None, one, ws, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_small(one, one, None, one, None, ws, 2, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_small(one, one, None, one, one, ws, 0, 64, 64, 8, 8, F16, None) == -1
    assert lib.conv3x3_small(one, one, None, one, one, ws, 2, 64, 64, 8, 8, 7, None) == -1
    assert lib.conv3x3_small(one, one, None, one, one, ws - 1, 2, 64, 64, 8, 8, F16, None) == -1  # workspace too small
    # fp32 and uncovered shapes
    assert lib.conv3x3_small(one, one, None, one, one, ws, 2, 64, 64, 8, 8, F32, None) == -5
    assert lib.conv3x3_small(one, one, None, one, one, ws, 2, 48, 64, 8, 8, F16, None) == -5
    # alignment
    assert lib.conv3x3_small(one + 2, one, None, one, one, ws, 2, 64, 64, 8, 8, F16, None) == -3
    assert lib.conv3x3_small(one, one, None, one + 8, one, ws, 2, 64, 64, 8, 8, F16, None) == -3
    # the pack
    assert lib.conv3x3_small_pack(None, one, 64, 64, 0, F16, None) == -1
    assert lib.conv3x3_small_pack(one, None, 64, 64, 0, F16, None) == -1
    assert lib.conv3x3_small_pack(one, one, 64, 64, 2, F16, None) == -1
    assert lib.conv3x3_small_pack(one, one, 64, 64, 0, 5, None) == -1
    assert lib.conv3x3_small_pack(one, one, 64, 64, 0, F32, None) == -5
    assert lib.conv3x3_small_pack(one, one, 64, 40, 1, F16, None) == -5
    assert lib.conv3x3_small_pack(one, one + 4, 64, 64, 0, F16, None) == -3


def test_the_front_keeps_cpu_and_fp32_calls_on_the_stock_line():
    from diffusion_finetuning_amd import conv

    x, w, b = torch.randn(1, 32, 4, 4), torch.randn(32, 32, 3, 3), torch.randn(32)
    ref = torch.nn.functional.conv2d(x, w, b, padding=1)
    assert torch.equal(conv.conv3x3(x, w, b), ref) and torch.equal(conv.conv3x3(x, w, b, route="stock"), ref)
    try:
        conv.conv3x3(x, w, b, route="hip")
        raise AssertionError("a CPU call must not be accepted by the forced route")
    except RuntimeError:
        pass
    layer = torch.nn.Conv2d(1280, 1280, 3, padding=1).requires_grad_(False)
    assert conv.prepack_conv3x3(layer) == 0  # nothing on a device: nothing to pack

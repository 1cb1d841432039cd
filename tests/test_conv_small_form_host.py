"""Host side of conv_small's staging forms (csrc/conv_small.hip): which form `conv3x3_small` takes for a shape, pinned to the
committed sweep log, and the refusals of `conv3x3_small_form` that are decided before any launch.  Runs without a device."""
import os
import re

import torch

from diffusion_finetuning_amd import _native as nat

F16, BF16, F32 = 1, 2, 0
POSITION, ROWS = 0, 1
UNSUPPORTED, BADARG = -5, -1


def _sweep_rows():
    """(side, C_in, C_out, {column: (median, spread)}) of the new tree's half of profiles/r18_conv_small_pipeline_sweep.log."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows, cols = [], None
    for line in open(os.path.join(root, "profiles", "r18_conv_small_pipeline_sweep.log")):
        if line.startswith("#  N"):
            cols = [c.strip() for c in re.findall(r"(fwd \w+|bwd \w+)", line)]
        m = re.match(r"\s+4\s+(\d+)x\d+\s+\d+\s+(\d+)\s+(\d+) \|", line)
        if m and cols and "fwd rows" in cols:
            vals = [(float(a), float(b)) for a, b in re.findall(r"([\d.]+) ±\s*([\d.]+)", line)]
            assert len(vals) == len(cols)
            rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), dict(zip(cols, vals))))
    return rows


def _parent_rows():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out, cols = {}, None
    for line in open(os.path.join(root, "profiles", "r18_conv_small_pipeline_sweep.log")):
        if line.startswith("#  N"):
            cols = [c.strip() for c in re.findall(r"(fwd \w+|bwd \w+)", line)]
        m = re.match(r"\s+4\s+(\d+)x\d+\s+\d+\s+(\d+)\s+(\d+) \|", line)
        if m and cols and "fwd hip" in cols:
            vals = [(float(a), float(b)) for a, b in re.findall(r"([\d.]+) ±\s*([\d.]+)", line)]
            out[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = dict(zip(cols, vals))
    return out


def test_the_default_form_is_the_sweeps_winner():
    """A class runs on the rows form only where the log shows it faster than the parent's kernel AND than the position form, in
    both directions, by more than the larger of the two spreads; the table of conv3x3_small_form_choice is that and no more."""
    rows, parent = _sweep_rows(), _parent_rows()
    assert len(rows) == 6 and len(parent) == 6
    for side, cin, cout, t in rows:
        p = parent[(side, cin, cout)]
        wins = all(t[d + " rows"][0] + max(t[d + " rows"][1], other[1]) < other[0]
                   for d in ("fwd", "bwd") for other in (p[d + " hip"], t[d + " position"]))
        want = ROWS if wins else POSITION
        for dtype in (torch.float16, torch.bfloat16):
            assert nat.conv3x3_small_form_choice(4, cin, cout, side, side, dtype) == want, (side, cin, cout)
            assert nat.conv3x3_small_form_choice(4, cout, cin, side, side, dtype) == want, (side, cout, cin)  # its backward class


def test_nothing_unmeasured_takes_the_rows_form():
    for shape in [(8, 1280, 1280, 8, 8), (4, 1280, 1280, 8, 16), (4, 320, 320, 8, 8), (4, 1280, 640, 8, 8), (2, 1280, 1280, 16, 16),
                  (4, 1280, 1280, 12, 12), (1, 32, 32, 1, 1), (65, 160, 32, 16, 16)]:
        assert nat.conv3x3_small_form_choice(*shape, torch.float16) == POSITION, shape
    assert nat.conv3x3_small_form_choice(4, 1280, 1280, 8, 8, torch.float32) == -1
    assert nat.lib().conv3x3_small_form_choice(4, 1280, 1300, 8, 8, F16) == -1  # channels off a multiple of 32: not covered


def test_refusals_come_before_any_launch():
    lib = nat.lib()
    p = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
    big = 1 << 40
    assert lib.conv3x3_small_form(p, p, None, p, p, big, 4, 64, 64, 8, 8, F16, 2, None) == BADARG
    assert lib.conv3x3_small_form(p, p, None, p, p, big, 4, 64, 64, 8, 8, F16, -1, None) == BADARG
    assert lib.conv3x3_small_form(None, p, None, p, p, big, 4, 64, 64, 8, 8, F16, ROWS, None) == BADARG
    assert lib.conv3x3_small_form(p, p, None, p, p, big, 4, 64, 64, 8, 8, F32, ROWS, None) == UNSUPPORTED
    # shapes the rows form does not cover: W off a multiple of 8, rows longer than a tile, the 64-pixel instantiation, tiles that
    # are neither whole images nor whole rows of one image
    for N, H, W in [(4, 12, 12), (1, 2, 280), (40, 1, 1), (4, 3, 8), (4, 24, 8)]:
        assert lib.conv3x3_small_supported(N, 64, 64, H, W, F16) == 1
        assert lib.conv3x3_small_form(p, p, None, p, p, big, N, 64, 64, H, W, F16, ROWS, None) == UNSUPPORTED, (N, H, W)
    # a covered shape gets as far as the workspace check
    assert lib.conv3x3_small_form(p, p, None, p, p, 0, 4, 64, 64, 8, 8, F16, ROWS, None) == BADARG
    assert lib.conv3x3_small_form(p, p, None, p, p + 2, big, 4, 64, 64, 16, 16, F16, ROWS, None) == -3  # LORA_E_ALIGN

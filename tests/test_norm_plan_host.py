"""`group_norm_act_plan`, the host-side query of how many kernels a fused GroupNorm call launches (csrc/norm.hip): 0 exactly where
the kernels refuse the shape, else 1 or 2, a function of its arguments alone.  The second half pins the plan of the 61 GroupNorm
sites of the sd15 UNet at the headline's batch of 4, so that a planner change shows up here as a diff."""
import itertools

from diffusion_finetuning_amd import _native as nat
from tests.norm_cases import BIG_GROUP, NCHW_GEOMETRY, NHWC_GEOMETRY, SMALL_GROUPS

# (N, C, HW, G): refused shapes next to accepted ones (the cases of test_norm_host's workspace test, and neighbours)
SHAPES = [(2, 16, 9, 4), (2, 16, 1, 4), (2, 12, 16, 4), (1, 512, 8, 512), (1, 257 * 8, 8, 257), (1, 256 * 8, 8, 256), (2, 18, 8, 4),
          (65536, 8, 8, 1), (0, 8, 8, 1), (2, 16, 8, 0), (2, 16, 8, 4), (4, 320, 4096, 32), (4, 1280, 64, 32), (1, 4096, 8, 1),
          (1, 4104, 8, 1), (3, 24, 24, 3), (2047, 32, 64, 32), (2048, 32, 64, 32)]
SHAPES += [(N, C, H * W, G) for N, C, G, H, W in NCHW_GEOMETRY + NHWC_GEOMETRY + [BIG_GROUP, SMALL_GROUPS]]


def _plan(*args):
    return nat.lib().group_norm_act_plan(*args)


def test_plan_is_zero_exactly_where_the_workspace_formula_is_and_one_or_two_otherwise():
    ws = nat.lib().group_norm_act_workspace_bytes
    seen = set()
    for (N, C, HW, G), cl, backward in itertools.product(SHAPES, (0, 1), (0, 1)):
        plan = _plan(N, C, HW, G, cl, backward)
        covered = ws(N, C, HW, G, cl, 0) > 0
        assert (plan == 0) == (not covered), (N, C, HW, G, cl, backward, plan)
        assert plan in ((1, 2) if covered else (0,)), (N, C, HW, G, cl, backward, plan)
        seen.add(plan)
    assert seen == {0, 1, 2}  # the list reaches every answer


def test_plan_is_deterministic_and_channels_last_always_takes_two_launches():
    for (N, C, HW, G), backward in itertools.product(SHAPES, (0, 1)):
        first = [_plan(N, C, HW, G, cl, backward) for cl in (0, 1)]
        for _ in range(3):
            assert [_plan(N, C, HW, G, cl, backward) for cl in (0, 1)] == first
        assert first[1] in (0, 2), (N, C, HW, G)


def test_plan_depends_only_on_slab_count_slab_size_and_direction():
    """What cannot matter: how N·G slabs of cpg·HW elements are split into N × G and cpg × HW, and any nonzero `backward` /
    `channels_last` value meaning the same as 1."""
    for slabs, cpg, HW in [(32, 40, 64), (128, 20, 1024), (128, 40, 1024), (256, 10, 4096), (256, 60, 1024), (64, 2, 16)]:
        for backward in (0, 1):
            base = _plan(1, slabs * cpg, HW, slabs, 0, backward)
            for N in (2, 4, 8, 32):  # the same slabs as N samples of slabs / N groups
                assert _plan(N, slabs // N * cpg, HW, slabs // N, 0, backward) == base, (slabs, cpg, HW, N)
            assert _plan(1, slabs * cpg * 2, HW // 2, slabs, 0, backward) == base  # twice the channels of half the rows
            assert _plan(1, slabs * cpg, HW, slabs, 0, 7 if backward else 0) == base
    assert _plan(2, 64, 64, 4, 5, 0) == _plan(2, 64, 64, 4, 1, 0) == 2


# the GroupNorm sites of the sd15 UNet on 64×64 latents as (C, H): how many there are, from harness/unet.py (ResNet norm1 / norm2,
# transformer entry norms, conv_norm_out); 32 groups each.  58 of them have a backward in the LoRA step (the others feed nothing
# trainable); the query does not know which, so both directions are listed for all 61.
SD15_SITES = {(320, 32): 1, (320, 64): 13, (640, 16): 1, (640, 32): 11, (640, 64): 2, (960, 32): 1, (960, 64): 1, (1280, 8): 12,
              (1280, 16): 11, (1280, 32): 1, (1920, 16): 1, (1920, 32): 1, (2560, 8): 3, (2560, 16): 2}
# slab KB (f16) → (forward, backward) launches at N = 4, i.e. 128 slabs: one launch up to 40 KB forward and 45 KB backward
SD15_PLAN_BATCH4 = {5: (1, 1), 10: (1, 1), 20: (1, 1), 30: (1, 1), 40: (1, 1), 60: (2, 2), 80: (2, 2), 120: (2, 2), 160: (2, 2),
                    240: (2, 2)}


def test_sd15_sites_at_batch_4_plan_as_recorded():
    assert sum(SD15_SITES.values()) == 61
    one = [0, 0]
    for (C, H), count in sorted(SD15_SITES.items()):
        kb = C // 32 * H * H * 2 // 1024
        got = tuple(_plan(4, C, H * H, 32, 0, backward) for backward in (0, 1))
        print(f"{count:2d} x C={C:4d} @ {H:2d}x{H:<2d} slab {kb:3d} KB: forward {got[0]} launch(es), backward {got[1]}")
        assert got == SD15_PLAN_BATCH4[kb], (C, H, kb, got)
        for d in (0, 1):
            one[d] += count * (got[d] == 1)
    assert one == [42, 42]  # the counts recorded in profiles/README.md, "GroupNorm in one launch"


def test_planner_limits_per_slab_count_are_the_recorded_ones():
    """Largest one-launch slab in 16-byte chunks (cpg·HW/8) per direction at 32, 128 and 256 slabs, and that slab counts in between
    and beyond take the limit of the measured count below them."""
    def limit(slabs, backward):
        # G = slabs groups of one channel each, HW = 8·chunks
        best, refused = 0, False
        for chunks in (1, 1280, 1281, 1920, 1921, 2560, 2561, 2880, 2881, 5120, 5121, 8192, 8193):
            if _plan(1, slabs, 8 * chunks, slabs, 0, backward) == 1:
                assert not refused, (slabs, chunks)  # monotonic: nothing above a size left on two launches is taken
                best = chunks
            else:
                refused = True
        return best

    assert [limit(s, 0) for s in (1, 32, 127, 128, 255, 256)] == [1920, 1920, 1920, 2560, 2560, 8192]
    assert [limit(s, 1) for s in (1, 32, 127, 128, 255, 256)] == [1280, 1280, 1280, 2880, 2880, 5120]
    assert _plan(8, 2048, 8 * 8192 // 64, 32, 0, 0) == 1  # 256 slabs of 64 channels × 128 chunks, the capacity itself

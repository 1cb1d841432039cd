"""Shapes (N, C, groups, H, W) that put the fused GroupNorm kernels (csrc/norm.hip) on every path of their planners and tails
that the workload's own shapes miss.  Plain data: the GPU tests (test_gpu_norm_edges.py) and the host tests of the workspace
formula (test_norm_host.py) share it.  The geometry in the comments is worked out by hand from the planner's formulas
(nchw_slices, nhwc_plan); no test reads the planner.

NCHW: one wave per (n,c) row, 4 rows per statistics workgroup, H·W/8 16-byte chunks per row on 64 lanes; the apply kernels cut
a group's cpg·H·W/8 chunks into `slices` = min(⌈2048/(N·G)⌉, ⌈chunks/512⌉) equal parts of ⌈chunks/slices⌉."""

NCHW_GEOMETRY = [
    (1, 6, 3, 2, 4),      # 6 rows: the second statistics workgroup has 2 of 4 waves past the end; 1 chunk per row (63 lanes idle)
    (3, 6, 6, 5, 8),      # cpg = 1: a group is one row, the fold has a single partial; 5 chunks per row
    (1, 8, 2, 20, 26),    # 65 chunks per row: the lane loop's second pass runs with lane 0 alone
    (1, 66, 2, 8, 17),    # 33·17 = 561 chunks per slab → 2 slices of 281: the boundary is in mid-row (281 = 16·17 + 9), 281 % 256 ≠ 0
    (2, 72, 1, 4, 4),     # cpg = 72 > 64: the fold's lane loop has a remainder pass of 8 lanes; G = 1
    (1, 264, 1, 2, 4),    # cpg = 264 > 256: the da loop's stride (256 threads) runs a second pass of 8
]

# NHWC: 512 threads = RP row lanes × C/8 channel columns (512 % (C/8) threads idle), S statistics row blocks and SA apply row
# blocks per sample: S = min(⌈256/N⌉, ⌈H·W/(4·RP)⌉, 64), SA = min(⌈1024/N⌉, ⌈H·W/(2·RP)⌉), each at least 1; a block has
# ⌈H·W/S⌉ rows, the last one what is left.
NHWC_GEOMETRY = [
    (2, 8, 1, 7, 9),        # C/8 = 1, RP = 512 > H·W = 63: 449 thread rows read nothing; S = SA = 1; one group of 8
    (2, 8, 2, 7, 9),        # the same with a thread's 8 channels in two groups
    (2, 8, 8, 7, 9),        # the same with cpg = 1: eight groups inside one thread
    (1, 4096, 256, 3, 3),   # C/8 = 512, RP = 1; G = 256 = kMaxGroups; S = 3 blocks of 3 rows, SA = 5 blocks of 2 (last: 1)
    (2, 24, 2, 1, 2),       # C/8 = 3, RP = 170, 2 threads idle; cpg = 12: group 0 ends inside thread 1's channels 8..15
    (2, 40, 8, 1, 127),     # C/8 = 5, RP = 102, 2 threads idle; cpg = 5: every thread straddles groups; 127 rows on 102 row lanes
    (1, 72, 8, 5, 5),       # C/8 = 9, RP = 56, 8 threads idle; cpg = 9; 25 rows on 56 row lanes
    (1, 64, 4, 7, 143),     # RP = 64, H·W = 1001: S = 4 blocks of 251 (last: 248), SA = 8 blocks of 126 (last: 119)
    (1, 512, 32, 48, 48),   # RP = 8, H·W = 2304: ⌈2304/32⌉ = 72 statistics blocks wanted, clipped to S = 64 of 36 rows; SA = 144 of 16
    (3, 320, 32, 6, 10),    # C/8 = 40, RP = 12, 32 threads idle; cpg = 10; S = 2 blocks of 30 rows, SA = 3 of 20
]

# the hard-statistics shapes: one group of 262 144 elements (NCHW: 64 rows of 4096, 64 apply slices; NHWC: RP = 64, S = 16 blocks
# of 256 rows, 4 rows per thread), and four small groups of 512 as the control
BIG_GROUP = (1, 64, 1, 64, 64)
SMALL_GROUPS = (2, 32, 4, 8, 8)

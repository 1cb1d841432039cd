"""Shapes and tables for the per-row gates of the fused forward (`lora_linear_fwd_rows`, csrc/lora_gemm.hip RS kernels).

No GPU and no library.  The shapes are the SMALLEST variant of every single-layer class of tests/gemm_cases.py::CASES with
its row count moved to the next multiple of RPS = 77 that keeps the class: one M then serves rows-per-sample 1 (a sample per
row), 77 (a sample boundary inside every 64- and 128-row tile and inside a 16-row fragment: 77 = 4·16 + 13) and M (one
sample).  tests/test_gpu_row_scales.py runs them; tests/test_row_scales_host.py checks this table on the CPU.
"""
import torch

from tests.gemm_cases import CASES, DTYPES, ESIZE, GENERIC, class_of

RPS = 77
RANKS = (1, 4, 16)
GENERIC_RANK = 20           # above the MFMA kernels' 16 slots: the shape-agnostic kernels whatever the alignment
GEGLU_SHAPE = (154, 64, 64)  # (M, K, F) of the gated `proj` launch: its smallest supported shape, two samples of 77 rows
NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}


def rows_variant(shape, esize):
    """`shape` with M replaced by the next multiple of RPS (>= M, >= 2·RPS) at which the launch class is still the shape's own."""
    key = class_of(shape, esize)
    M = max((shape[0] + RPS - 1) // RPS, 2) * RPS  # (at least two samples of RPS rows: a boundary to get wrong)
    for _ in range(64):
        cand = (M,) + tuple(shape[1:])
        if class_of(cand, esize) == key:
            return cand
        M += RPS
    raise AssertionError(("no multiple of %d keeps the class" % RPS, key, shape))


def operator_cases():
    """[(key, shape, dtype, rank)]: every class × every dtype it exists for × RANKS (+ GENERIC_RANK on the generic class)."""
    out = []
    for esize, table in CASES.items():
        for key, shapes in table.items():
            shape = rows_variant(shapes[0], esize)
            for dtype in DTYPES[esize]:
                for r in RANKS + ((GENERIC_RANK,) if key[0] == GENERIC else ()):
                    out.append((key, shape, dtype, r))
    return out


def sample_counts(M):
    """n_samples for rows-per-sample 1, RPS and M."""
    assert M % RPS == 0
    return (M, M // RPS, 1)


def case_id(key, shape, dtype, r):
    return "%s-%s%dx%ds%d-%s%s-r%d" % (NAME[dtype], key[0], key[1], key[2], key[3], "x".join(map(str, shape[:3])),
                                       "-offset" if len(shape) > 3 else "", r)


def mixed_table(n_samples, R, values, seed):
    """A gate table whose sample i is CLOSED (all zeros) for i % 3 == 1 and else filled with one of `values`, the open samples
    taking them in turn — so every sample boundary separates two different factors.  Returns (table, which): which[i] = -1 for
    a closed sample, else the index into `values`."""
    which = torch.tensor([-1 if i % 3 == 1 else (i - (i + 1) // 3 + seed) % len(values) for i in range(n_samples)])
    table = torch.zeros(n_samples, R)
    for v, value in enumerate(values):
        table[which == v] = value
    return table, which


def one_hot_table(assign, slots, R):
    """table[b, slots[assign[b]]] = 1, zero elsewhere."""
    table = torch.zeros(len(assign), R)
    for b, k in enumerate(assign.tolist()):
        table[b, slots[k]] = 1.0
    return table


assert ESIZE  # (re-exported for the tests)

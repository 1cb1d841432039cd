"""Shapes of tests/test_gpu_attention_f32.py.  INSTANTIATIONS names one (B, Tq, Tk, H, d) per compiled instantiation of
csrc/attn_f32.hip — its dispatch key is DF, the head dim's width in 16-column chunks — and
tests/test_attention_f32_host.py checks that its keys are exactly that file's dispatch table."""

# (B, Tq, Tk, H, d, multiplier of Q and K): tile edges, not the workload
OPERATOR_SHAPES = [
    (2, 200, 300, 2, 64, 1.0),    # several key tiles, ragged query block
    (2, 70, 90, 2, 40, 1.0),      # d % 16 == 8
    (1, 130, 77, 2, 160, 1.0),    # the cross-attention key count, widest head
    (1, 257, 257, 1, 8, 1.0),     # one past a block boundary, narrowest head
    (2, 96, 77, 3, 80, 3.0),      # odd head count: head/batch strides; sharper softmax
    (1, 5, 1, 1, 16, 1.0),        # a single key: O == V
    (1, 1, 513, 2, 64, 1.0),      # a single query row
    (1, 1100, 1100, 1, 64, 1.0),  # many key tiles: the online rescale chain
    (1, 70, 130, 1, 128, 1.0),    # the DF = 8 instantiation (no shape above reaches it)
]


def df_of(d):
    """Mirror of plan_f32 (csrc/attn_f32.hip): the narrowest compiled width 16·DF that holds the head dim."""
    for top, df in ((32, 2), (48, 3), (64, 4), (96, 6), (128, 8), (160, 10)):
        if d <= top:
            return df
    raise ValueError(d)


INSTANTIATIONS = {
    2: (1, 257, 257, 1, 8),
    3: (2, 70, 90, 2, 40),
    4: (2, 200, 300, 2, 64),
    6: (2, 96, 77, 3, 80),
    8: (1, 70, 130, 1, 128),
    10: (1, 130, 77, 2, 160),
}

"""CPU-only guards for the fused-GEMM edge tests (tests/test_gpu_gemm_edges.py):

1. the case table of tests/gemm_cases.py names exactly the `launch_tile` instantiations that a single-layer launch of
   csrc/lora_gemm.hip can reach, per element size — a tile class added to the dispatch without a case, or a case for a
   class that is gone, fails here;
2. the dispatch mirrors send every table shape to its key and reach nothing outside the table, and they are pinned, line
   by line, to the C++ they copy — a threshold moved there fails here instead of moving a case to another kernel;
3. the three-part check `assert_close` accepts a correctly rounded result and rejects four plausible GEMM bugs at exactly
   the bounds the GPU file uses, for f16 and bf16."""
import os
import re

import pytest
import torch

from oracle import lora_oracle as orc
from tests.gemm_cases import (CASES, FALLBACK, GENERIC, RING, SKINNY_CASES, SPLIT, class_of, gate_tile_width,
                              gemm_launch_class, make_layer, plan_splitk, skinny_class_of, skinny_launch_class)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion_finetuning_amd", "csrc")
SRC = os.path.join(CSRC, "lora_gemm.hip")  # plan_splitk, gate_tile_width, launch_tile, launch_pipe, launch_typed
# ... followed by what it includes: kRowBytes lives with the kernel, kRP and kVec in common.h
INCLUDED = ("lora_gemm_kernel.h", "common.h")
TILE = re.compile(r"launch_tile<T,\s*(\d+),\s*(\d+),\s*(true|false),\s*(\d+)(?:,\s*\d+)*>")


def _source():
    text = ""
    for path in (SRC, *(os.path.join(CSRC, name) for name in INCLUDED)):
        with open(path) as f:
            text += f.read()
    return text


def _body(src, start, end):
    """The text from the line that begins a function to the line that begins the next definition."""
    i = src.index(start)
    return src[i:src.index(end, i)]


def _block(body, opener):
    """(the brace block that `opener` opens, the body without it): blocks of launch_pipe close at their opener's indent."""
    i = body.index(opener)
    indent = len(body[:i]) - len(body[:i].rstrip(" "))
    close = "\n" + " " * indent + "}\n"
    j = body.index(close, i) + len(close)
    return body[i:j], body[:i] + body[j:]


def _tiles(text):
    return {(int(bm), int(bn), main == "true", int(stg)) for bm, bn, main, stg in TILE.findall(text)}


def compiled_classes():
    """{esize: (main classes, skinny classes)} that launch_typed / launch_pipe hand out when tile_part is null."""
    src = _source()
    pipe = _body(src, "int launch_pipe(const GemmParams& p", "struct CallArgs")
    typed = _body(src, "int launch_typed(const CallArgs& c", "int launch_gemm(")
    _, pipe = _block(pipe, "if (p.tile_part != nullptr) {")   # grouped launches: tests/test_gpu_groups.py
    split, pipe = _block(pipe, "if (p.splitk > 1) {")
    half, rest = _block(pipe, "if constexpr (sizeof(T) == 2) {")
    fallback = {t for t in _tiles(typed) if t[3] == 0}
    assert _tiles(typed) == fallback and {t[2] for t in fallback} == {True, False}, "launch_typed launches the two fallback tiles"
    generic = set()
    if "lora_gemm_generic_kernel<T>" in typed and "lora_skinny_generic_kernel<T>" in typed:
        generic = {(GENERIC, 0, 0, 0)}
    out = {}
    for esize in (2, 4):
        ring = _tiles(rest) | (_tiles(half) if esize == 2 else set())
        main = {(RING, bm, bn, stg) for bm, bn, m, stg in ring if m}
        main |= {(SPLIT, bm, bn, stg) for bm, bn, m, stg in _tiles(split) if m}
        main |= {(FALLBACK, bm, bn, stg) for bm, bn, m, stg in fallback if m} | generic
        skinny = {(RING, bm, bn, stg) for bm, bn, m, stg in ring if not m}
        skinny |= {(FALLBACK, bm, bn, stg) for bm, bn, m, stg in fallback if not m} | generic
        out[esize] = (main, skinny)
    return out


def test_every_reachable_instantiation_has_a_case():
    compiled = compiled_classes()
    # (the parse sees what it should: eight ring tiles for 16-bit types, four for f32, two split tiles, one skinny tile)
    assert len([c for c in compiled[2][0] if c[0] == RING]) == 8 and len([c for c in compiled[4][0] if c[0] == RING]) == 4
    assert {c for c in compiled[2][0] if c[0] == SPLIT} == {(SPLIT, 64, 128, 3), (SPLIT, 128, 128, 2)}
    for esize in (2, 4):
        main, skinny = compiled[esize]
        table = {k[:4] for k in CASES[esize]}
        assert len(table) == len(CASES[esize]), "one key per class"
        assert table == main, (esize, "untested", main - table, "not compiled", table - main)
        sk = {k[:4] for k in SKINNY_CASES[esize]}
        assert sk == skinny, (esize, "untested", skinny - sk, "not compiled", sk - skinny)
    # f32 cannot enter launch_pipe's sizeof(T) == 2 block
    only16 = {k[:4] for k in CASES[2]} - {k[:4] for k in CASES[4]}
    assert only16 == {(RING, 64, 160, 2), (RING, 128, 160, 2), (RING, 64, 128, 2), (RING, 64, 128, 3)}


def test_every_case_reaches_its_class_and_the_mirror_reaches_nothing_else():
    for esize, table in CASES.items():
        for key, shapes in table.items():
            for shape in shapes:
                assert class_of(shape, esize) == key, (esize, key, shape, class_of(shape, esize))
            if key[0] in (RING, SPLIT):  # a ragged last row tile, and a ragged last column tile where the rule admits one
                assert any(s[0] % key[1] for s in shapes), (key, "no ragged M")
                if not (key[2] == 160 or key[:4] == (RING, 64, 128, 3)):
                    assert any(s[2] % key[2] for s in shapes), (key, "no ragged Nc")
        for key, shapes in SKINNY_CASES[esize].items():
            for shape in shapes:
                assert skinny_class_of(shape, esize) == key, (esize, key, shape)
    # everything check_common accepts (M >= 1, K, N >= 1; the rank only has to fit), on a coarse grid
    ms = (1, 63, 64, 65, 128, 200, 1000, 2000, 4000, 8100, 8192, 13100, 16330, 16384, 32768, 40000)
    ks = (1, 4, 8, 32, 36, 50, 64, 72, 96, 128, 256, 288, 512, 576, 1280, 1536, 1568, 1696, 3072, 3136, 3392, 5120, 10240)
    ns = (1, 4, 8, 50, 64, 68, 72, 128, 136, 160, 200, 320, 512, 640, 960, 1000, 1024, 1280, 2560, 5120, 10240)
    for esize in (2, 4):
        reach, sk = set(), set()
        for M in ms:
            for Kc in ks:
                sk |= {skinny_launch_class(M, Kc, esize, a)[:4] for a in (True, False)}
                for Nc in ns:
                    for aligned in (True, False):
                        for ws in (True, False):
                            reach.add(gemm_launch_class(M, Kc, Nc, esize, aligned, ws)[:4])
        assert reach == {k[:4] for k in CASES[esize]}, (esize, reach ^ {k[:4] for k in CASES[esize]})
        assert sk == {k[:4] for k in SKINNY_CASES[esize]}


def test_split_cases_have_uneven_slices():
    for esize, table in CASES.items():
        for key, shapes in table.items():
            if key[0] != SPLIT:
                continue
            M, Kc, Nc = shapes[0]
            S, bm = plan_splitk(M, Kc, Nc, esize)
            nk = Kc * esize // 128
            assert (S, bm) == (key[4], key[1]) and nk % S != 0, (key, S, bm, nk)  # the last slice is shorter than the others


def test_mirrors_match_the_cpp_they_copy():
    """gemm_launch_class, plan_splitk and gate_tile_width of tests/gemm_cases.py copy launch_typed, plan_splitk, launch_pipe
    and gate_tile_width; pin every line that decides a class."""
    src = _source()
    plan = _body(src, "SplitPlan plan_splitk(", "int64_t splitk_ws_bytes(")
    for line in ("SplitPlan off{1, 128};",
                 "const int nk = (Kc * esize + kRowBytes - 1) / kRowBytes;",
                 "const int64_t tiles128 = ((M + 127) / 128) * ((Nc + 127) / 128);",
                 "const int64_t tiles64 = ((M + 63) / 64) * ((Nc + 127) / 128);",
                 "if ((Nc & 7) != 0 || (Kc * esize) % kRowBytes != 0 || tiles128 >= 192) return off;",
                 "if (nk < 48) return off;",
                 "int bm = tiles128 <= 96 ? 64 : 128;",
                 "if (tiles128 >= 64 && nk >= 128) bm = 128;",
                 "const int64_t tiles = bm == 64 ? tiles64 : tiles128;",
                 "if (tiles > kTicketBytes / 4) return off;",
                 "int S = (int)((480 + tiles / 2) / tiles);",
                 "if (S > 8) S = 8;",
                 "const int min_steps = 10;",
                 "while (S > 1 && nk / S < min_steps) --S;",
                 "while (S > 1 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;",
                 "return SplitPlan{S, bm};"):
        assert line in plan, line
    assert len(re.findall(r"\breturn\b", plan)) == 4 and len(re.findall(r"\bbm = ", plan)) == 2  # no branch the mirror lacks
    assert "constexpr int kRowBytes = 128;" in src and "constexpr int kRP = 16;" in src
    assert "constexpr int kTicketBytes = LORA_GEMM_WS_TICKET_BYTES;" in src
    with open(os.path.join(os.path.dirname(SRC), "..", "..", "include", "lora_hip.h")) as f:
        assert "#define LORA_GEMM_WS_TICKET_BYTES 4096" in f.read()

    gate = _body(src, "int gate_tile_width(", "template <typename T, int BN>")
    for line in ("if (cols % 160 != 0) return 128;",
                 "const int64_t t128 = tiles_m * (cols / 128), t160 = tiles_m * (cols / 160);",
                 "if (gated) return t128 > 256 && t128 < 2048 ? 160 : 128;",
                 "const double c128 = (double)((t128 + 511) / 512), c160 = 1.25 * (double)((t160 + 511) / 512);",
                 "return c160 < c128 ? 160 : 128;"):
        assert line in gate, line

    pipe = _body(src, "int launch_pipe(const GemmParams& p", "struct CallArgs")
    code = "\n".join(l.split("//")[0].rstrip() for l in pipe.splitlines())  # (its comments hold measurements, not rules)
    for line in ("if (!MAIN) return launch_tile<T, 64, 64, false, 3>(p, stream);",
                 "if (p.splitk > 1) {",
                 "if (p.split_bm == 64) return launch_tile<T, 64, 128, true, 3, 4>(p, stream);",
                 "return launch_tile<T, 128, 128, true, 2, 4>(p, stream);",
                 "const int64_t tiles128 = ((p.M + 127) / 128) * ((p.Nc + 127) / 128);",
                 "const int64_t tiles64 = ((p.M + 63) / 64) * ((p.Nc + 63) / 64);",
                 "const int padded = (p.Nc + 127) / 128 * 128;",
                 "const bool p128 = p.n_parts == 0 || (p.part_n % 128) == 0, p160 = p.n_parts == 0 || (p.part_n % 160) == 0;",
                 "const bool big = tiles128 >= 128 && (padded - p.Nc) * 4 <= p.Nc && p128;",
                 "if constexpr (sizeof(T) == 2) {",
                 "const int64_t tiles160 = ((p.M + 127) / 128) * (p.Nc / 160);",
                 "const bool w160 = (p.Nc % 160) == 0 && ((p.Nc % 128) != 0 || !p128) && tiles160 >= 128 && p160;",
                 "if (w160 && tiles160 < 384) return launch_tile<T, 64, 160, true, 2, 4>(p, stream);",
                 "if (w160) return launch_tile<T, 128, 160, true, 2, 4>(p, stream);",
                 "if (big && tiles128 < 256) return launch_tile<T, 64, 128, true, 2, 4>(p, stream);",
                 "if (!big && tiles128 >= 64 && (p.Nc % 128) == 0 && p128) return launch_tile<T, 64, 128, true, 3, 4>(p, stream);",
                 "if (big && p160 && tiles128 >= 256 && gate_tile_width((p.M + 127) / 128, p.Nc, false) == 160)",
                 "return launch_tile<T, 128, 160, true, 2, 4>(p, stream);",
                 "if (big) return launch_tile<T, 128, 128, true, 2, 4>(p, stream);",
                 "const bool deep = tiles64 < 512;",
                 "const int nk = (p.Kc * (int)sizeof(T) + kRowBytes - 1) / kRowBytes;",
                 "int ring = deep ? 3 : 2;",
                 "if (deep && nk >= 8) ring = 4;",
                 "case 4: return launch_tile<T, 64, 64, true, 4>(p, stream);",
                 "case 3: return launch_tile<T, 64, 64, true, 3>(p, stream);",
                 "default: return launch_tile<T, 64, 64, true, 2>(p, stream);"):
        assert line in code, line
    # no return the mirror lacks: the twelve pinned above and the one of the tile_part branch (grouped launches)
    assert len(re.findall(r"\breturn\b", code)) == 13, len(re.findall(r"\breturn\b", code))

    typed = _body(src, "int launch_typed(const CallArgs& c", "int launch_gemm(")
    for line in ("constexpr int VEC = ElemTraits<T>::kVec;",
                 "constexpr int BK = kRowBytes / (int)sizeof(T);",
                 "const bool fast = c.r <= kRP && c.Fp != nullptr && (c.Qp != nullptr || !main_part) && (c.Kc % VEC) == 0 &&",
                 "(lda % VEC) == 0 && aligned16(c.Am) && aligned16(c.Fp) && aligned16(c.Qp) &&",
                 "(!main_part || ((c.Nc % VEC) == 0 && aligned16(c.Bm) && aligned16(c.C)));",
                 "if (main_part && !grouped && c.workspace != nullptr && aligned16(c.workspace) && (c.Kc % BK) == 0) {",
                 "const SplitPlan sp = plan_splitk(c.M, c.Kc, c.Nc, (int)sizeof(T));",
                 "if (sp.S > 1 && c.ws_bytes >= splitk_ws_bytes(c.M, c.Nc, sp)) {",
                 "if ((c.Kc % BK) == 0) return main_part ? launch_pipe<T, true>(p, stream) : launch_pipe<T, false>(p, stream);",
                 "return main_part ? launch_tile<T, 64, 64, true, 0>(p, stream) : launch_tile<T, 64, 64, false, 0>(p, stream);"):
        assert line in typed, line
    with open(os.path.join(os.path.dirname(SRC), "common.h")) as f:
        common = f.read()
    assert len(re.findall(r"static constexpr int kVec = 8;", common)) == 2 and "static constexpr int kVec = 4;" in common
    # the kernel kinds the GPU file tells apart
    tile = _body(src, "int launch_tile(GemmParams p", "int gate_tile_width(")
    for line in ("const int blocks = p.tiles_m * p.tiles_n * p.splitk;",
                 "return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM, 0, true>, lds, PK_GEMM_SPLITK>(blocks, NW * 64, p, stream);",
                 "if (rs) return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM, 0, true, 1, true>, lds, PK_GEMM_SPLITK>(blocks, NW * 64, p, stream);",
                 "constexpr int prof_id = MAIN ? (BM >= 256 ? PK_GEMM_256x128 : (BM == 128 ? PK_GEMM_128x128 : PK_GEMM_64x64))",
                 ": (BM == 128 ? PK_SKINNY_128 : PK_SKINNY_64);"):
        assert line in tile, line
    assert gate_tile_width(103, 640) == 160 and gate_tile_width(32, 1000) == 128


# ---- sensitivity of assert_close at the bounds of tests/test_gpu_gemm_edges.py -----------------------------------------

TOL = {torch.float16: 1e-3, torch.bfloat16: 1e-2}  # tests/test_gpu_parity.py's TOL, which the GPU file imports
M, K, N, R, SCALE = 130, 72, 200, 8, 0.7           # a fallback case of the table: every edge of it is ragged
assert (M, K, N) in CASES[2][(FALLBACK, 64, 64, 0, 1)]


def _forward(x, w, b, down, up):
    return orc.lora_linear_forward(x.double(), w.double(), None if b is None else b.double(), down.double(), up.double(), SCALE)


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def planted(request):
    """The float64 forward of the case on operands rounded to the dtype (what the GPU file feeds the kernel), and four
    wrong results a GEMM kernel could plausibly produce at its edges."""
    dtype = request.param
    x, w, b, down, up, _ = make_layer(M, K, N, R, dtype, seed=1)
    y = _forward(x, w, b, down, up)
    bugs = {}
    bad = y.clone()   # (1) a row clamp off by one: the last valid row of the last row tile is computed from row M-2
    bad[M - 1] = y[M - 2]
    bugs["last row from row M-2"] = bad
    bad = y.clone()   # (2) the last 8 columns receive no rank-r term
    bad[:, N - 8:] = _forward(x, w, b, down, up * 0)[:, N - 8:]
    bugs["no rank-r term in the last 8 columns"] = bad
    k_full = K // 64 * 64  # (3) the last, partial K-step of the fallback contraction is dropped (16-bit K-steps hold 64)
    bugs["partial K-step dropped"] = _forward(x[:, :k_full], w[:, :k_full], b, down[:, :k_full], up)
    bad = y.clone()   # (4) no bias on the last column tile
    n0 = (N - 1) // 64 * 64
    bad[:, n0:] = _forward(x, w, None, down, up)[:, n0:]
    bugs["no bias on the last column tile"] = bad
    return dtype, y, bugs


def test_assert_close_accepts_a_correctly_rounded_gemm(close, planted):
    dtype, y, _ = planted
    close(y.to(dtype), y, TOL[dtype])


def test_assert_close_rejects_planted_gemm_bugs(close, planted):
    dtype, y, bugs = planted
    assert len(bugs) == 4
    for name, bad in bugs.items():
        with pytest.raises(AssertionError):
            close(bad.to(dtype), y, TOL[dtype], name)

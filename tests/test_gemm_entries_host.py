"""CPU-only pins of the fused-GEMM entry points (csrc/lora_gemm.hip, csrc/lora_pack.hip): what a move of the host code could
break without any other test noticing.

1. `lora_gemm_workspace_bytes` — the compiled plan_splitk and splitk_ws_bytes — against the mirror of tests/gemm_cases.py on
   the grid of test_gemm_coverage_host.test_every_case_reaches_its_class_and_the_mirror_reaches_nothing_else;
2. the status every entry returns BEFORE its first HIP call, one row per distinct early return and per pair of checks whose
   order shows in the status.  Pointers are made-up integers that the library compares and never dereferences: every row
   returns before a launch (LORA_E_LAUNCH appears nowhere, and LORA_OK only where nothing is launched: M == 0, or a rank
   that lora_pack_factors leaves to the generic kernels)."""
import pytest

from diffusion_finetuning_amd import _native as nat
from tests.gemm_cases import TICKET_BYTES, plan_splitk

OK, BADARG, RANK, LAUNCH, UNSUPPORTED = 0, -1, -2, -4, -5
F32, F16, BF16 = 0, 1, 2

# the grid of test_gemm_coverage_host.py: everything check_common accepts, coarse
MS = (1, 63, 64, 65, 128, 200, 1000, 2000, 4000, 8100, 8192, 13100, 16330, 16384, 32768, 40000)
KS = (1, 4, 8, 32, 36, 50, 64, 72, 96, 128, 256, 288, 512, 576, 1280, 1536, 1568, 1696, 3072, 3136, 3392, 5120, 10240)
NS = (1, 4, 8, 50, 64, 68, 72, 128, 136, 160, 200, 320, 512, 640, 960, 1000, 1024, 1280, 2560, 5120, 10240)


def test_workspace_bytes_follow_the_split_plan():
    fn = nat.lib().lora_gemm_workspace_bytes
    points = split = 0
    for dtype, esize in ((F32, 4), (F16, 2), (BF16, 2)):
        for M in MS:
            for Kc in KS:
                for Nc in NS:
                    S, bm = plan_splitk(M, Kc, Nc, esize)
                    want = 0
                    if S > 1:  # [tickets | S fp32 slabs of a bm×128 tile and its bm×16 P tile, per tile]
                        want = TICKET_BYTES + -(-M // bm) * -(-Nc // 128) * S * (bm * 128 + bm * 16) * 4
                        split += 1
                    points += 1
                    assert fn(M, Kc, Nc, dtype) == want, (M, Kc, Nc, dtype, S, bm)
    assert points == 23184 and split > 1000, (points, split)
    assert fn(0, 1280, 1280, F16) == 0 and fn(1024, 0, 1280, F16) == 0 and fn(1024, 10240, 0, F16) == 0


# Made-up addresses: P (16-byte aligned, one per argument so that none aliases), P + 1 (unaligned), P + 4 (4- but not 8-byte).
P = 0x7F0000010000
ARGS = {  # entry -> its arguments in order, with values that pass every check (such a call would launch: no row uses one as is)
    "lora_linear_fwd_ws": dict(X=P, W=P + 0x100, bias=None, A=P + 0x200, B=P + 0x300, Apack=P + 0x400, Bpack=P + 0x500,
                               Y=P + 0x600, T=P + 0x700, M=4, K=8, N=8, r=2, scale=1.0, dtype=F16, ws=None, ws_bytes=0,
                               stream=None),
    "lora_linear_fwd_rows": dict(X=P, W=P + 0x100, bias=None, A=P + 0x200, B=P + 0x300, Apack=P + 0x400, Bpack=P + 0x500,
                                 Y=P + 0x600, T=P + 0x700, M=4, K=8, N=8, r=2, scale=1.0, table=P + 0x800, n_samples=2, ld=2,
                                 dtype=F16, ws=None, ws_bytes=0, stream=None),
    "lora_linear_geglu_fwd": dict(X=P, W=P + 0x100, bias=None, Apack=P + 0x400, Bpack=P + 0x500, Y=P + 0x600, Out=P + 0x900,
                                  T=P + 0x700, M=4, K=64, N=128, r=2, scale=1.0, dtype=F16, stream=None),
    "lora_linear_geglu_fwd_rows": dict(X=P, W=P + 0x100, bias=None, Apack=P + 0x400, Bpack=P + 0x500, Y=P + 0x600,
                                       Out=P + 0x900, T=P + 0x700, M=4, K=64, N=128, r=2, scale=1.0, table=P + 0x800,
                                       n_samples=2, ld=2, dtype=F16, stream=None),
    "geglu_linear_bwd": dict(dZ=P, W2t=P + 0x100, Y=P + 0x600, dY=P + 0x900, zeros=P + 0xA00, M=4, Nz=64, F=128, dtype=F16,
                             stream=None),
    "lora_linear_bwd_input_ws": dict(dY=P, Wt=P + 0x100, A=P + 0x200, B=P + 0x300, Apack=P + 0x400, Bpack=P + 0x500,
                                     dX=P + 0x600, U=P + 0x700, M=4, K=8, N=8, r=2, scale=1.0, dtype=F16, ws=None, ws_bytes=0,
                                     stream=None),
    "lora_gemm_packed": dict(Am=P, lda=0, Bm=P + 0x100, bias=None, Fp=P + 0x400, Qp=P + 0x500, tile_part=None,
                             part_table=None, n_parts=0, C=P + 0x600, P_out=P + 0x700, M=4, Kc=64, Nc=64, r=2, scale=1.0,
                             work_cols=0, ws=None, ws_bytes=0, dtype=F16, stream=None),
    "lora_gemm_parts": dict(Am=P, Bm=P + 0x100, bias=None, Fp=P + 0x400, Qp=P + 0x500, C=P + 0x600, P_out=P + 0x700, ldp=6,
                            M=4, Kc=192, Nc=192, r=2, n_parts=3, on_k=0, scale=1.0, dtype=F16, stream=None),
    "lora_pack_factors": dict(A=P + 0x200, B=P + 0x300, Apack=P + 0x400, Bpack=P + 0x500, K=32, N=32, r=2, dtype=F16,
                              stream=None),
    "lora_pack_factors_batched": dict(table=P + 0x800, n=1, max_len=32, params=P + 0x200, packed=P + 0x400, dtype=F16,
                                      stream=None),
    "lora_pack_items": dict(table=P + 0x800, n=1, max_len=32, params=P + 0x200, packed=P + 0x400, dtype=F16, stream=None),
}

_SIZES = [(dict(M=-1), BADARG), (dict(K=0), BADARG), (dict(N=0), BADARG)]
_DTYPE = [(dict(dtype=7), BADARG), (dict(dtype=-1), BADARG)]
_RANK = [(dict(r=0), RANK), (dict(r=9, K=8, N=64), RANK), (dict(r=9, K=64, N=8), RANK),
         (dict(r=0, dtype=7), BADARG), (dict(r=0, N=0), BADARG),     # size and dtype are looked at before the rank
         (dict(M=0, r=0), RANK)]                                      # ... and the rank before the empty batch
_EMPTY_FWD = dict(M=0, X=None, W=None, A=None, B=None, Apack=None, Bpack=None, Y=None, T=None)
_EMPTY_GEGLU = dict(M=0, X=None, W=None, Apack=None, Bpack=None, Y=None, Out=None, T=None)
_TABLE = [(dict(table=None), BADARG), (dict(n_samples=0), BADARG), (dict(n_samples=3), BADARG), (dict(ld=1), BADARG),
          (dict(table=None, r=0), RANK),            # check_common first
          (dict(table=None, M=0), BADARG),          # the table is checked before the empty batch returns
          (dict(n_samples=3, X=None), BADARG)]

_ADDRESS = {k: v for args in ARGS.values() for k, v in args.items() if isinstance(v, int) and v >= P}  # (by argument name)


def _nulls(*names):
    return [({name: None}, BADARG) for name in names]


def _unaligned(*names):
    return [({name: _ADDRESS[name] + 1}, UNSUPPORTED) for name in names]

_GEGLU_UNSUPPORTED = ([(dict(dtype=F32), UNSUPPORTED), (dict(Apack=None), UNSUPPORTED),
                       (dict(Bpack=None), UNSUPPORTED), (dict(K=72), UNSUPPORTED), (dict(N=64), UNSUPPORTED),
                       (dict(bias=P + 0xB04), UNSUPPORTED), (dict(Y=None, X=P + 1), UNSUPPORTED)]
                      + _unaligned("X", "W", "Apack", "Bpack", "Out", "Y")
                      + [(dict(dtype=F32, X=None), BADARG)])  # a null operand is reported before the missing kernel

TABLE = {
    "lora_linear_fwd_ws": _SIZES + _DTYPE + _RANK + [(_EMPTY_FWD, OK)] + _nulls("X", "W", "A", "B", "Y", "T"),
    "lora_linear_fwd_rows": (_SIZES + _DTYPE + _RANK + _TABLE + [(_EMPTY_FWD, OK), (dict(_EMPTY_FWD, n_samples=3), OK)]
                             + _nulls("X", "W", "A", "B", "Y", "T")),
    "lora_linear_geglu_fwd": (_SIZES + _DTYPE + _RANK
                              + [(dict(N=127), BADARG), (dict(N=127, M=0), BADARG), (dict(N=7, K=8, r=8), RANK),
                                 (dict(N=127, dtype=F32), BADARG), (_EMPTY_GEGLU, OK), (dict(_EMPTY_GEGLU, dtype=F32), OK)]
                              + _nulls("X", "W", "Out", "T") + _GEGLU_UNSUPPORTED + [(dict(r=17), UNSUPPORTED)]),
    "lora_linear_geglu_fwd_rows": (_SIZES + _DTYPE + _RANK + _TABLE
                                   + [(dict(N=127), BADARG), (dict(N=7, K=8, r=8, table=None), RANK),
                                      (dict(table=None, dtype=F32), BADARG),    # the table before the missing kernel
                                      (dict(n_samples=3, K=72), BADARG), (_EMPTY_GEGLU, OK)]
                                   + _nulls("X", "W", "Out", "T") + _GEGLU_UNSUPPORTED
                                   + [(dict(r=17, ld=17), UNSUPPORTED), (dict(r=17), BADARG)]),  # (a 2-wide table: too narrow)
    "geglu_linear_bwd": ([(dict(M=-1), BADARG), (dict(Nz=0), BADARG), (dict(F=0), BADARG)] + _DTYPE
                         + [(dict(M=0, dZ=None, W2t=None, Y=None, dY=None, zeros=None), OK), (dict(M=0, dtype=F32, F=64), OK)]
                         + _nulls("dZ", "W2t", "Y", "dY", "zeros")
                         + [(dict(dtype=F32), UNSUPPORTED), (dict(Nz=96), UNSUPPORTED), (dict(F=64), UNSUPPORTED),
                            (dict(dtype=F32, dZ=None), BADARG)]
                         + _unaligned("dZ", "W2t", "Y", "dY", "zeros")),
    "lora_linear_bwd_input_ws": (_SIZES + _DTYPE + _RANK
                                 + [(dict(M=0, dY=None, Wt=None, A=None, B=None, dX=None, U=None), OK)]
                                 + _nulls("dY", "A", "B", "U", "Wt") + [(dict(Wt=None, dX=None, U=None), BADARG)]),
    "lora_gemm_packed": ([(dict(M=-1), BADARG), (dict(Kc=0), BADARG), (dict(r=0), BADARG), (dict(r=17), BADARG)] + _DTYPE
                         + [(dict(M=0, Am=None, Fp=None, Bm=None, Qp=None), OK), (dict(M=0, r=17), BADARG)]
                         + _nulls("Am", "Fp", "Bm", "Qp") + [(dict(Nc=0), BADARG)]
                         + [(dict(C=None, tile_part=P + 0xC00), BADARG),                      # tile_part: MAIN launches only
                            (dict(part_table=P + 0xD00, n_parts=2), BADARG),                  # part_table: skinny launches only
                            (dict(C=None, part_table=P + 0xD00, n_parts=0), BADARG),
                            (dict(Am=P + 1, Fp=None), BADARG)]
                         # only packed factors behind the call: whatever the ring or fallback kernels do not take is unsupported
                         + [(dict(Am=P + 1), UNSUPPORTED), (dict(Fp=P + 0x401), UNSUPPORTED), (dict(Qp=P + 0x501), UNSUPPORTED),
                            (dict(Bm=P + 0x101), UNSUPPORTED), (dict(C=P + 0x601), UNSUPPORTED), (dict(Kc=68), UNSUPPORTED),
                            (dict(Nc=68), UNSUPPORTED), (dict(lda=68), UNSUPPORTED), (dict(dtype=F32, Kc=66), UNSUPPORTED),
                            (dict(C=None, Am=P + 1), UNSUPPORTED), (dict(C=None, Fp=P + 0x401), UNSUPPORTED),
                            # grouped launches exist on the ring only: a ragged contraction has no kernel
                            (dict(Kc=72, tile_part=P + 0xC00), UNSUPPORTED),
                            (dict(C=None, Kc=72, part_table=P + 0xD00, n_parts=2), UNSUPPORTED)]),
    "lora_gemm_parts": ([(dict(M=-1), BADARG), (dict(Kc=0), BADARG), (dict(Nc=0), BADARG), (dict(r=0), BADARG),
                         (dict(r=17, ldp=64), BADARG), (dict(n_parts=1), BADARG), (dict(n_parts=5, ldp=10), BADARG)] + _DTYPE
                        + [(dict(M=0, Am=None, Bm=None, Fp=None, Qp=None, C=None, P_out=None, ldp=0), OK)]
                        + _nulls("Am", "Bm", "Fp", "Qp", "C", "P_out")
                        + [(dict(ldp=5), BADARG), (dict(Nc=128), BADARG), (dict(on_k=1, Kc=128), BADARG),
                           (dict(Nc=128, dtype=F32), BADARG), (dict(ldp=5, Am=P + 1), BADARG)]
                        + [(dict(dtype=F32), UNSUPPORTED), (dict(Nc=96), UNSUPPORTED), (dict(Kc=96), UNSUPPORTED),
                           (dict(on_k=1, Nc=12), UNSUPPORTED), (dict(bias=P + 0xB04), UNSUPPORTED)]
                        + _unaligned("Am", "Bm", "Fp", "Qp", "C")
                        + [(dict(on_k=1, n_parts=2, Kc=128, ldp=4), UNSUPPORTED),   # the part-wise backward exists for 3 parts
                           (dict(on_k=1, n_parts=4, Kc=256, ldp=8), UNSUPPORTED)]),
    "lora_pack_factors": (_nulls("A", "B", "Apack", "Bpack")
                          + [(dict(K=0), BADARG), (dict(N=0), BADARG), (dict(r=0), RANK), (dict(r=33), RANK),
                             (dict(r=9, K=8), RANK), (dict(r=0, A=None), BADARG),
                             (dict(r=17), OK), (dict(r=17, dtype=7), OK),          # left to the generic kernels: nothing to pack
                             (dict(dtype=7), BADARG), (dict(r=16, dtype=3), BADARG)]),
    "lora_pack_factors_batched": (_nulls("table", "params", "packed")
                                  + [(dict(n=0), BADARG), (dict(max_len=0), BADARG), (dict(dtype=7), BADARG),
                                     (dict(dtype=-1), BADARG)]),
    "lora_pack_items": (_nulls("table", "params", "packed")
                        + [(dict(n=0), BADARG), (dict(max_len=0), BADARG), (dict(dtype=7), BADARG), (dict(dtype=-1), BADARG)]),
}

ROWS = [(entry, over, want) for entry, rows in TABLE.items() for over, want in rows]


def test_the_table_covers_every_entry_and_launches_nothing():
    assert set(TABLE) == set(ARGS) and len(ROWS) > 250
    for entry, over, want in ROWS:
        assert over and set(over) <= set(ARGS[entry]), (entry, over)
        assert want in (OK, BADARG, RANK, UNSUPPORTED) and want != LAUNCH
        if want == OK:  # ... only where the entry has nothing to launch
            assert over.get("M") == 0 or (entry == "lora_pack_factors" and over["r"] > 16), (entry, over)
    for entry, rows in TABLE.items():  # every entry: every distinct early status it has
        has = {want for _, want in rows}
        assert BADARG in has and (OK in has or entry.startswith("lora_pack_")), entry
        assert (RANK in has) == (entry not in ("geglu_linear_bwd", "lora_gemm_packed", "lora_gemm_parts",
                                               "lora_pack_factors_batched", "lora_pack_items")), entry
        assert (UNSUPPORTED in has) == (entry in ("lora_linear_geglu_fwd", "lora_linear_geglu_fwd_rows", "geglu_linear_bwd",
                                                   "lora_gemm_packed", "lora_gemm_parts")), entry


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_status_before_any_launch(entry):
    fn = getattr(nat.lib(), entry)
    for over, want in TABLE[entry]:
        args = dict(ARGS[entry], **over)
        assert fn(*args.values()) == want, (entry, over, want)

"""Every conv route through ``conv_fwd`` / ``conv_dgrad`` / ``conv_wgrad``
against a float64 reference on the CPU, with an elementwise bound that has
no free constants (the form tests/test_conv_dgrad_strided.py,
tests/test_conv_wgrad_px.py and tests/test_gemm_exact.py use):

    ref = float64 conv2d / conv2d_input / conv2d_weight of the inputs
    mag = the same of their absolute values
    |got - ref| <= n 2^-23 mag + store |ref|

n is the reduction length (KH KW Cin for fwd, KH KW Cout for dgrad, N HO WO
for wgrad). n 2^-23 mag is the (n-1) u sum|t_i| summation bound with
u = 2^-24, doubled for MFMA-internal rounding, atomic order and the rounded
products of the fp32 kernels; it holds for any summation order. ``store`` is
2^-8, the unit roundoff of one round-to-nearest bf16 store, and 0 for an fp32
result. An element with a zero bound must be exactly zero.

bf16 cases use bf16-valued inputs (their products are exact in fp32); fp32
cases use inputs that are NOT bf16-representable, so a kernel that narrows
its operands fails.

Every case first asserts the route (``conv_route``, csrc/conv_route.h;
tests/test_conv_route.py derives the rules and checks this table without a
GPU), so a gate change cannot quietly turn a case into a test of another
kernel. CASES says what each shape is for.

``test_bound_is_sharp`` (no GPU) shows on the small cases that the bound is
neither loose nor unfair: fp32 arithmetic emulated on the CPU stays within
it, and each of five single-defect mutants of the reference exceeds it.

Measured worst error / bound on an MI355X, per route (the store term
dominates a bf16 result, so an honest kernel sits just under 1 there; the
CPU emulation gives 0.92 - 0.99 and 0.001 - 0.03 on the same inputs, a
truncating store 1.8 - 2.0, narrowed operands 20 - 100):

    route            op      bf16 result      fp32 result
    Halo             fwd     0.81 - 0.96
    Halo             dgrad   0.82 - 0.96
    Conv8            fwd     0.93 - 0.99
    Conv8            dgrad   0.93 - 0.99
    Generic          fwd     0.90 - 0.99      0.005 - 0.052
    Generic          dgrad   0.74 - 0.99      0.002 - 0.032
    DgradPhase       dgrad   0.49 (7x7 stem; more in test_conv_dgrad_strided)
    WgradPx          wgrad   0.99             0.017
    WgradGeneric     wgrad   0.92 - 0.98      0.001 - 0.011
    Wgrad1x1SplitK   wgrad   0.89 - 0.96      0.001 - 0.023
    Wgrad1x1Slab     wgrad   0.90 - 0.91      0.001

Writing the 1x3 and padded-1x1 cases found a bug by reading: the forward
stager took its dense-GEMM shortcut (output row m = x row m) for every
KH == 1 stride-1 conv, also a 1xKW kernel or a padded 1x1, whose rows are
shifted pixels and outnumber the pixels of x. Fixed in conv.hip (the shortcut
now needs KW == 1 and pad == 0); ``gen_fwd_1x3_*`` and ``gen_fwd_1x1_pad1_*``
cover it."""

import functools

import pytest
import torch
import torch.nn.functional as F

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32


def case(op, N, H, W, Cin, Cout, K, s, p, dtype=BF16, poison=False, **route):
    """K: int or (KH, KW). poison: a NaN block of the output's size goes back
    to the allocator just before the call. ``route`` holds the expected
    conv_route entries, derived by hand."""
    KH, KW = (K, K) if isinstance(K, int) else K
    return dict(op=op, N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, s=s,
                p=p, dtype=dtype, poison=poison, route=route)


def halo(gx, gy):      # grid: 128-pixel tiles x 64-filter tiles
    return dict(kind="Halo", tile=(128, 64), grid=(gx, gy, 1))


def gen(bn, gx, gy, fast):   # grid: column tiles x 128-pixel tiles
    return dict(kind="Generic", tile=(128, bn), grid=(gx, gy, 1), fast=fast,
                use_swz=0)


def c8(gx, gy):        # grid: 256-column tiles x 256-pixel tiles
    return dict(kind="Conv8", tile=(256, 256), grid=(gx, gy, 1), use_swz=1)


def wg(bm, gx, gy, splits, p_chunk):
    return dict(kind="WgradGeneric", tile=(bm, 128), grid=(gx, gy, splits),
                splits=splits, p_chunk=p_chunk, transpose_dy=True,
                transpose_x=False)


def wg1x1(kind, gemm_kind, tile, grid, p_chunk):
    return dict(kind=kind, gemm_kind=gemm_kind, tile=tile, grid=grid,
                splits=grid[2], p_chunk=p_chunk, transpose_dy=True,
                transpose_x=kind == "Wgrad1x1Slab")


CASES = {
    # ---- halo kernel, fwd: gate bf16 3x3 s1 p1, 128 % W == 0,
    # H*W % 128 == 0, Cin % 32 == 0, Cout % 64 == 0 ----
    # one tile is the whole image
    "halo_fwd_16x8": case("fwd", 2, 16, 8, 32, 64, 3, 1, 1, poison=True,
                          **halo(2, 1)),
    # non-square, odd N, three k-steps
    "halo_fwd_8x16_odd_n_3k": case("fwd", 3, 8, 16, 96, 64, 3, 1, 1,
                                   **halo(3, 1)),
    "halo_fwd_4x32_co192": case("fwd", 1, 4, 32, 32, 192, 3, 1, 1,
                                **halo(1, 3)),
    "halo_fwd_32x4": case("fwd", 2, 32, 4, 32, 64, 3, 1, 1, **halo(2, 1)),
    # R == H == 2
    "halo_fwd_2x64": case("fwd", 2, 2, 64, 32, 64, 3, 1, 1, **halo(2, 1)),
    # every row is all halo above and below
    "halo_fwd_1x128": case("fwd", 2, 1, 128, 32, 64, 3, 1, 1, **halo(2, 1)),
    # one pixel per row: every pixel has halo left and right
    "halo_fwd_128x1": case("fwd", 1, 128, 1, 32, 64, 3, 1, 1, **halo(1, 1)),
    # eight tiles per image: interior tiles whose halo rows are real data
    "halo_fwd_32x32_n1": case("fwd", 1, 32, 32, 96, 192, 3, 1, 1,
                              **halo(8, 3)),
    # ---- halo kernel, dgrad: Cout % 32 == 0, Cin % 64 == 0 ----
    "halo_dgrad_16x8": case("dgrad", 2, 16, 8, 64, 32, 3, 1, 1, poison=True,
                            **halo(2, 1)),
    "halo_dgrad_8x16_odd_n_3k": case("dgrad", 3, 8, 16, 64, 96, 3, 1, 1,
                                     **halo(3, 1)),
    "halo_dgrad_4x32_ci192": case("dgrad", 1, 4, 32, 192, 32, 3, 1, 1,
                                  **halo(1, 3)),
    "halo_dgrad_32x4": case("dgrad", 2, 32, 4, 64, 32, 3, 1, 1, **halo(2, 1)),
    "halo_dgrad_2x64": case("dgrad", 2, 2, 64, 64, 32, 3, 1, 1, **halo(2, 1)),
    "halo_dgrad_1x128": case("dgrad", 2, 1, 128, 64, 32, 3, 1, 1,
                             **halo(2, 1)),
    "halo_dgrad_32x32_n1": case("dgrad", 1, 32, 32, 192, 96, 3, 1, 1,
                                **halo(8, 3)),
    # ---- just outside each clause of the halo gate: generic kernel ----
    "nohalo_fwd_fp32": case("fwd", 2, 16, 8, 32, 64, 3, 1, 1, FP32,
                            **gen(64, 1, 2, True)),
    "nohalo_fwd_8x8": case("fwd", 2, 8, 8, 32, 64, 3, 1, 1,       # H*W = 64
                           **gen(64, 1, 1, True)),
    "nohalo_fwd_w12": case("fwd", 1, 32, 12, 32, 64, 3, 1, 1,     # 3 * 128 px
                           **gen(64, 1, 3, True)),
    "nohalo_fwd_cin48": case("fwd", 2, 16, 8, 48, 64, 3, 1, 1,
                             **gen(64, 1, 2, False)),
    "nohalo_fwd_cout96": case("fwd", 2, 16, 8, 32, 96, 3, 1, 1,
                              **gen(128, 1, 2, True)),
    # pad 0: 14 x 6 outputs, 168 rows
    "nohalo_fwd_pad0": case("fwd", 2, 16, 8, 32, 64, 3, 1, 0,
                            **gen(64, 1, 2, True)),
    # stride 2: 8 x 4 outputs, 64 rows
    "nohalo_fwd_stride2": case("fwd", 2, 16, 8, 32, 64, 3, 2, 1,
                               **gen(64, 1, 1, True)),
    "nohalo_dgrad_8x8": case("dgrad", 2, 8, 8, 64, 32, 3, 1, 1,
                             **gen(64, 1, 1, True)),
    "nohalo_dgrad_cout48": case("dgrad", 2, 16, 8, 64, 48, 3, 1, 1,
                                **gen(64, 1, 2, False)),
    "nohalo_dgrad_cin96": case("dgrad", 2, 16, 8, 96, 32, 3, 1, 1,
                               **gen(128, 1, 2, True)),
    "nohalo_dgrad_fp32": case("dgrad", 2, 16, 8, 64, 32, 3, 1, 1, FP32,
                              **gen(64, 1, 2, True)),
    # ---- conv8, fwd: bf16, Cout % 256 == 0, Cin % 32 == 0, K % 64 == 0,
    # ceil(M / 256) * Cout / 256 >= 256 ----
    # K = 64: two k-halves, the prologue is shorter than 3; M = 32768
    "c8_fwd_1x1_two_khalves": case("fwd", 512, 8, 8, 64, 512, 1, 1, 0,
                                   **c8(2, 128)),
    # 2x2 pad 1 on 7x7 -> 8x8 outputs: the tap cursor advances every k-half
    "c8_fwd_2x2_tap_per_khalf": case("fwd", 1024, 7, 7, 32, 256, 2, 1, 1,
                                     **c8(1, 256)),
    # 3x3 on 8x8 skips the halo kernel (64 px per image): padding zeros come
    # from the zero page
    "c8_fwd_3x3_8x8": case("fwd", 512, 8, 8, 64, 512, 3, 1, 1, poison=True,
                           **c8(2, 128)),
    # stride 2: 2622 images of 5x5 outputs = 65550 rows = 256 tiles + 14 rows,
    # and 257 blocks: ragged last tile, uneven XCD remap (257 % 8 == 1)
    "c8_fwd_stride2_ragged": case("fwd", 2622, 8, 8, 32, 256, 2, 2, 1,
                                  **c8(1, 257)),
    # 2641 images of 4x4 -> 5x5 outputs = 66025 rows = 257 tiles + 233 rows,
    # 258 blocks (258 % 8 == 2)
    "c8_fwd_ragged_xcd": case("fwd", 2641, 4, 4, 32, 256, 2, 1, 1,
                              **c8(1, 258)),
    # ---- conv8, dgrad: stride 1, Cin % 256 == 0, Cout % 32 == 0 ----
    "c8_dgrad_1x1_two_khalves": case("dgrad", 512, 8, 8, 512, 64, 1, 1, 0,
                                     **c8(2, 128)),
    "c8_dgrad_3x3_8x8": case("dgrad", 1024, 8, 8, 256, 64, 3, 1, 1,
                             poison=True, **c8(1, 256)),
    # pad 0: HO = 4 != H = 6; 1821 * 36 = 65556 rows = 256 tiles + 20 rows
    "c8_dgrad_3x3_pad0_ragged": case("dgrad", 1821, 6, 6, 256, 64, 3, 1, 0,
                                     **c8(1, 257)),
    # 2x2 pad 1 (HO = 5 > H = 4); 4097 * 16 = 65552 rows, 257 blocks
    "c8_dgrad_2x2_ragged_xcd": case("dgrad", 4097, 4, 4, 256, 32, 2, 1, 1,
                                    **c8(1, 257)),
    # ---- just outside the conv8 gate ----
    # 255 row tiles x 1 column tile
    "noc8_fwd_255_blocks": case("fwd", 1020, 8, 8, 64, 256, 1, 1, 0,
                                **gen(128, 2, 510, True)),
    # K = 32: a single k-half
    "noc8_fwd_k32": case("fwd", 1024, 8, 8, 32, 256, 1, 1, 0,
                         **gen(128, 2, 512, True)),
    "noc8_dgrad_255_blocks": case("dgrad", 1020, 8, 8, 256, 64, 1, 1, 0,
                                  **gen(128, 2, 510, True)),
    # ---- stride-2 dgrad kernel on the stem's 7x7 (the 3x3 / 1x1 cases are
    # in tests/test_conv_dgrad_strided.py): class rows 56 / 48 / 49 / 42 ----
    "phase_dgrad_7x7": case("dgrad", 1, 15, 13, 3, 64, 7, 2, 3, poison=True,
                            kind="DgradPhase", tile=(128, 64),
                            grid=(4, 1, 1)),
    # ---- pixel-major wgrad (the rest is in tests/test_conv_wgrad_px.py) ----
    "px_wgrad_one_step": case("wgrad", 2, 4, 4, 64, 64, 3, 1, 1, poison=True,
                              kind="WgradPx", tile=(64, 64), grid=(1, 1, 1),
                              splits=1, p_chunk=32, transpose_dy=False),
}

# ---- generic fwd / stride-1 dgrad, bf16 and fp32 ----
for dt, tag in ((BF16, "bf16"), (FP32, "fp32")):
    CASES.update({
        # stem: Cin = 3, K = 27 < one k-step
        f"gen_fwd_stem_{tag}": case("fwd", 2, 8, 8, 3, 64, 3, 1, 1, dt,
                                    poison=dt is BF16,
                                    **gen(64, 1, 1, False)),
        # 7x7 s2 p3, odd H and W: 8 x 7 outputs; K = 147
        f"gen_fwd_7x7_{tag}": case("fwd", 1, 15, 13, 3, 64, 7, 2, 3, dt,
                                   **gen(64, 1, 1, False)),
        # Cin = 40: K = 360, a k-step spans taps and the last one is 8 wide;
        # Cout = 72: ragged 128-column tile
        f"gen_fwd_cin40_cout72_{tag}": case("fwd", 1, 9, 9, 40, 72, 3, 1, 1,
                                            dt, **gen(128, 1, 1, False)),
        # FAST, 147 rows: a full tile and a ragged one
        f"gen_fwd_cin32_ragged_m_{tag}": case("fwd", 3, 7, 7, 32, 64, 3, 1, 1,
                                              dt, **gen(64, 1, 2, True)),
        # Cout = 200: two column tiles, the second 72 wide; stride 2 on odd
        # H and W
        f"gen_fwd_cout200_s2_{tag}": case("fwd", 2, 9, 9, 32, 200, 3, 2, 1,
                                          dt, **gen(128, 2, 1, True)),
        # pad 0: 5 x 5 outputs, 75 rows
        f"gen_fwd_pad0_{tag}": case("fwd", 3, 7, 7, 32, 64, 3, 1, 0, dt,
                                    **gen(64, 1, 1, True)),
        # pad 2 with a 3x3 kernel: 8x8 outputs from 6x6 inputs
        f"gen_fwd_pad2_{tag}": case("fwd", 1, 6, 6, 32, 64, 3, 1, 2, dt,
                                    **gen(64, 1, 1, True)),
        # 1x1 stride 1, N = 1: the full first tile stages as a dense GEMM
        # slice (bf16), the ragged second tile by the gather
        f"gen_fwd_1x1_{tag}": case("fwd", 1, 12, 12, 64, 128, 1, 1, 0, dt,
                                   **gen(128, 1, 2, True)),
        # 1x3 pad 1 and a padded 1x1: KH == 1 and stride 1 but NOT a dense
        # GEMM (7 x 6 and 7 x 8 outputs from 5 x 6 inputs, 168 / 224 rows)
        f"gen_fwd_1x3_{tag}": case("fwd", 4, 5, 6, 32, 64, (1, 3), 1, 1, dt,
                                   **gen(64, 1, 2, True)),
        f"gen_fwd_1x1_pad1_{tag}": case("fwd", 4, 5, 6, 32, 64, 1, 1, 1, dt,
                                        **gen(64, 1, 2, True)),
        # dgrad. Stem: 3 output columns
        f"gen_dgrad_stem_{tag}": case("dgrad", 2, 8, 8, 3, 64, 3, 1, 1, dt,
                                      poison=dt is BF16,
                                      **gen(64, 1, 1, True)),
        # Cout = 40: non-FAST, K = 360; Cin = 72 ragged column tile
        f"gen_dgrad_cout40_cin72_{tag}": case("dgrad", 1, 9, 9, 72, 40, 3, 1,
                                              1, dt, **gen(128, 1, 1, False)),
        f"gen_dgrad_cin200_{tag}": case("dgrad", 2, 7, 7, 200, 32, 3, 1, 1,
                                        dt, **gen(128, 2, 1, True)),
        # pad 0: HO = 5 < H = 7; 147 rows
        f"gen_dgrad_pad0_{tag}": case("dgrad", 3, 7, 7, 64, 32, 3, 1, 0, dt,
                                      **gen(64, 1, 2, True)),
        # pad 2: HO = 8 > H = 6
        f"gen_dgrad_pad2_{tag}": case("dgrad", 1, 6, 6, 64, 32, 3, 1, 2, dt,
                                      **gen(64, 1, 1, True)),
        f"gen_dgrad_1x1_{tag}": case("dgrad", 1, 12, 12, 128, 64, 1, 1, 0, dt,
                                     **gen(128, 1, 2, True)),
        f"gen_dgrad_1x3_{tag}": case("dgrad", 4, 5, 6, 64, 32, (1, 3), 1, 1,
                                     dt, **gen(64, 1, 1, True)),
    })

# ---- wgrad outside the pixel-major kernel; each runs with an fp32 and a
# bf16 result. Generic: column tiles = ceil(KH KW Cin / 128), row tiles =
# ceil(Cout / bm), want = min(ceil(P / 32), 512 / tiles), p_chunk =
# ceil(P / want) rounded up to 32, splits = ceil(P / p_chunk) ----
CASES.update({
    # 3x3 s2 on 9x9: P = 50; 5 x 1 tiles; want 2 -> chunk 32, last slice 18
    "wg_3x3_s2": case("wgrad", 2, 9, 9, 64, 128, 3, 2, 1, poison=True,
                      **wg(128, 5, 1, 2, 32)),
    # 1x1 s2: P = 50, 64-row tile
    "wg_1x1_s2": case("wgrad", 2, 9, 9, 64, 64, 1, 2, 0,
                      **wg(64, 1, 1, 2, 32)),
    # stem: 27 columns; P = 128 -> 4 slices of one k-step
    "wg_stem": case("wgrad", 2, 8, 8, 3, 64, 3, 1, 1, **wg(64, 1, 1, 4, 32)),
    # 7x7 s2 p3: 147 columns, P = 56
    "wg_7x7": case("wgrad", 1, 15, 13, 3, 64, 7, 2, 3,
                   **wg(64, 2, 1, 2, 32)),
    # fp32 3x3 s1: the pixel-major kernel is bf16 only
    "wg_fp32": case("wgrad", 2, 8, 8, 64, 64, 3, 1, 1, FP32,
                    **wg(64, 5, 1, 4, 32)),
    # odd extents, ragged tiles both ways (360 columns, 136 rows): P = 105,
    # 3 x 2 tiles -> want min(4, 85) = 4, chunk 32, last slice 9 pixels
    "wg_odd_cout136": case("wgrad", 3, 7, 5, 40, 136, 3, 1, 1,
                           **wg(128, 3, 2, 4, 32)),
    # short last split: 18 x 2 tiles -> target 512 / 36 = 14; P = 30 * 16 =
    # 480 = 15 k-steps -> want 14, chunk = ceil(480 / 14) = 35 -> 64, so the
    # grid has ceil(480 / 64) = 8 slices, the last one half full
    "wg_short_last_split": case("wgrad", 30, 8, 8, 256, 256, 3, 2, 1,
                                **wg(128, 18, 2, 8, 64)),
    # 1x1 stride 1 = a GEMM dw[Cout, Cin] over K = P (gemm_plan.h). P = 50:
    # 128x64 tile, two slices of 32 and 18
    "wg_1x1_splitk_small": case(
        "wgrad", 2, 5, 5, 64, 64, 1, 1, 0, poison=True,
        **wg1x1("Wgrad1x1SplitK", "TwoPhaseSplitK", (128, 64), (1, 1, 2),
                32)),
    # P = 392 = 12 slices of 32 and one of 8; Cin = 72 ragged
    "wg_1x1_splitk_ragged": case(
        "wgrad", 8, 7, 7, 72, 128, 1, 1, 0,
        **wg1x1("Wgrad1x1SplitK", "TwoPhaseSplitK", (128, 64), (2, 1, 13),
                32)),
    "wg_1x1_splitk_fp32": case(
        "wgrad", 2, 5, 5, 64, 64, 1, 1, 0, FP32,
        **wg1x1("Wgrad1x1SplitK", "TwoPhaseSplitK", (128, 64), (1, 1, 2),
                32)),
    # slab route: Cin = Cout = 256 and the smallest P with slab_splits > 1
    # (two slices of kSlabMinChunk = 256)
    "wg_1x1_slab_p512": case(
        "wgrad", 8, 8, 8, 256, 256, 1, 1, 0, poison=True,
        **wg1x1("Wgrad1x1Slab", "G9Slab", (256, 256), (1, 1, 2), 256)),
    # P = 576: two slices of 288 = 9 k-halves, the g8 kernel
    "wg_1x1_slab_p576_g8": case(
        "wgrad", 9, 8, 8, 256, 256, 1, 1, 0,
        **wg1x1("Wgrad1x1Slab", "G8Slab", (256, 256), (1, 1, 2), 288)),
    # P = 520: 260 is no multiple of 32 -> no slab; 4 x 2 tiles of 128 x 64,
    # 17 slices
    "wg_1x1_p520_no_slab": case(
        "wgrad", 130, 2, 2, 256, 256, 1, 1, 0,
        **wg1x1("Wgrad1x1SplitK", "TwoPhaseSplitK", (128, 64), (4, 2, 17),
                32)),
})

# (case, out_f32): wgrad runs both ways; out_f32 means nothing elsewhere
RUNS = [(name, f32) for name, c in CASES.items()
        for f32 in ((True, False) if c["op"] == "wgrad" else (False,))]

# the small cases the CPU test works through
SHARP_RUNS = [
    ("halo_fwd_16x8", False), ("halo_dgrad_16x8", False),
    ("gen_fwd_stem_bf16", False), ("gen_fwd_7x7_fp32", False),
    ("gen_fwd_cin40_cout72_fp32", False), ("gen_fwd_cout200_s2_bf16", False),
    ("gen_dgrad_pad0_bf16", False), ("gen_dgrad_cout40_cin72_fp32", False),
    ("gen_dgrad_pad2_bf16", False),
    ("wg_3x3_s2", True), ("wg_3x3_s2", False), ("wg_stem", False),
    ("wg_fp32", True), ("wg_1x1_splitk_small", False),
    ("px_wgrad_one_step", True),
]


def reduction_length(c):
    HO, WO = out_hw(c)
    return {"fwd": c["KH"] * c["KW"] * c["Cin"],
            "dgrad": c["KH"] * c["KW"] * c["Cout"],
            "wgrad": c["N"] * HO * WO}[c["op"]]


def out_hw(c):
    return ((c["H"] + 2 * c["p"] - c["KH"]) // c["s"] + 1,
            (c["W"] + 2 * c["p"] - c["KW"]) // c["s"] + 1)


def result_dtype(c, out_f32):
    return FP32 if (out_f32 or c["dtype"] is FP32) else BF16


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_cpu(c, a, b):
    """The op of case c on NHWC / OHWI operands (fwd: x, w; dgrad: dy, w;
    wgrad: dy, x), in the operands' dtype, result NHWC / OHWI."""
    s, p = c["s"], c["p"]
    if c["op"] == "fwd":
        return nhwc(F.conv2d(nchw(a), nchw(b), stride=s, padding=p))
    if c["op"] == "dgrad":
        return nhwc(torch.nn.grad.conv2d_input(
            (c["N"], c["Cin"], c["H"], c["W"]), nchw(b), nchw(a), stride=s,
            padding=p))
    return nhwc(torch.nn.grad.conv2d_weight(
        nchw(b), (c["Cout"], c["Cin"], c["KH"], c["KW"]), nchw(a), stride=s,
        padding=p))


@functools.lru_cache(maxsize=4)
def problem(name):
    """Inputs, float64 reference and summation bound on the CPU; computed
    once per case and never modified."""
    c = CASES[name]
    HO, WO = out_hw(c)
    g = torch.Generator().manual_seed(
        97 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    x_shape = (c["N"], c["H"], c["W"], c["Cin"])
    y_shape = (c["N"], HO, WO, c["Cout"])
    w_shape = (c["Cout"], c["KH"], c["KW"], c["Cin"])
    a_shape, b_shape = {"fwd": (x_shape, w_shape), "dgrad": (y_shape, w_shape),
                        "wgrad": (y_shape, x_shape)}[c["op"]]
    a = torch.randn(a_shape, generator=g)
    b = torch.randn(b_shape, generator=g)
    if c["dtype"] is BF16:
        a, b = a.to(BF16), b.to(BF16)
    else:
        # an fp32 case whose inputs a bf16 kernel would compute exactly
        # proves nothing
        assert (a.to(BF16).float() != a).float().mean() > 0.9
        assert (b.to(BF16).float() != b).float().mean() > 0.9
    ref = conv_cpu(c, a.double(), b.double())
    mag = conv_cpu(c, a.double().abs(), b.double().abs())
    bsum = reduction_length(c) * 2.0 ** -23 * mag
    return a, b, ref, bsum


def worst_ratio(got, ref, bsum, store):
    err = (got.double() - ref).abs()
    lim = bsum + store * ref.abs()
    # an element with a zero bound must be exactly 0
    return torch.where(lim > 0, err / lim, (err > 0).double() * 2).max().item()


def assert_route(name):
    c = CASES[name]
    got = OPS.conv_route(c["op"], c["N"], c["H"], c["W"], c["Cin"], c["Cout"],
                         c["KH"], c["KW"], c["s"], c["p"],
                         bf16=c["dtype"] is BF16)
    assert got["out_hw"] == out_hw(c), (name, got)
    for key, val in c["route"].items():
        assert got[key] == val, f"{name}: {key} is {got[key]!r}, want {val!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,out_f32", RUNS)
def test_conv_exact(name, out_f32):
    c = CASES[name]
    assert_route(name)
    a, b, ref, bsum = problem(name)
    a_d, b_d = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    res_dtype = result_dtype(c, out_f32)
    if c["poison"]:
        junk = torch.full(tuple(ref.shape), float("nan"), dtype=res_dtype,
                          device=DEV)
        del junk
    if c["op"] == "fwd":
        got = OPS.conv_fwd(a_d, b_d, c["s"], c["p"])
    elif c["op"] == "dgrad":
        got = OPS.conv_dgrad(a_d, b_d, c["H"], c["W"], c["s"], c["p"])
    else:
        got = OPS.conv_wgrad(a_d, b_d, c["KH"], c["KW"], c["s"], c["p"],
                             out_f32)
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == res_dtype
    got = got.cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite result"
    ratio = worst_ratio(got, ref, bsum, 2.0 ** -8 if res_dtype is BF16 else 0.0)
    print(f"conv exact {c['route']['kind']} {c['op']} {name} "
          f"{'f32' if res_dtype is FP32 else 'bf16'} out: "
          f"worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error is {ratio:.3f} x the bound"


# ---- the bound itself, without a GPU ---------------------------------------

def store(t, res_dtype):
    """What an honest kernel's epilogue does to an fp32 / exact value."""
    return t.to(res_dtype)


def truncate_bf16(t32):
    bits = t32.contiguous().view(torch.int32) & -65536      # 0xFFFF0000
    return bits.view(torch.float32).to(BF16)                # exact


def first_tap(c, want_padding):
    """(ho, wo, kh, kw, hi, wi): an output pixel of image 0 and a tap whose
    input position (hi, wi) is outside the image (want_padding) or inside."""
    HO, WO = out_hw(c)
    for ho in range(HO):
        for wo in range(WO):
            for kh in range(c["KH"]):
                for kw in range(c["KW"]):
                    hi = ho * c["s"] - c["p"] + kh
                    wi = wo * c["s"] - c["p"] + kw
                    inside = 0 <= hi < c["H"] and 0 <= wi < c["W"]
                    # inside: take a tap in the middle of the image
                    if inside and not want_padding and ho >= HO // 2 \
                            and wo >= WO // 2:
                        return ho, wo, kh, kw, hi, wi
                    if not inside and want_padding:
                        return ho, wo, kh, kw, hi, wi
    return None


def tap_term(c, a, b, tap, chans):
    """The contribution of ONE (output pixel, tap) pair of image 0 to the
    result, restricted to the contracted channels ``chans`` (fwd / dgrad) or
    to the input channels ``chans`` (wgrad), with the input pixel clamped
    into the image: (index of the touched result slice, float64 term)."""
    ho, wo, kh, kw, hi, wi = tap
    hi = min(max(hi, 0), c["H"] - 1)
    wi = min(max(wi, 0), c["W"] - 1)
    a, b = a.double(), b.double()
    if c["op"] == "fwd":       # a = x, b = w: y[0, ho, wo, :]
        return (0, ho, wo), b[:, kh, kw, chans] @ a[0, hi, wi, chans]
    if c["op"] == "dgrad":     # a = dy, b = w: dx[0, hi, wi, :]
        return (0, hi, wi), a[0, ho, wo, chans] @ b[chans, kh, kw, :]
    # wgrad: a = dy, b = x: dw[:, kh, kw, chans]
    return ((slice(None), kh, kw, chans),
            torch.outer(a[0, ho, wo, :], b[0, hi, wi, chans]))


def contracted_slot(c):
    """One 8-channel slot of the contraction (all of it for the stem)."""
    n = {"fwd": c["Cin"], "dgrad": c["Cout"], "wgrad": c["Cin"]}[c["op"]]
    lo = 8 if n >= 16 else 0
    return slice(lo, min(lo + 8, n))


@pytest.mark.parametrize("name,out_f32", SHARP_RUNS)
def test_bound_is_sharp(name, out_f32):
    """fp32 arithmetic (float32 conv on the CPU, result rounded to bf16 where
    the kernel stores bf16) meets the bound, and every single-defect mutant
    exceeds it: the bound separates a right kernel from a subtly wrong one
    on these inputs."""
    c = CASES[name]
    a, b, ref, bsum = problem(name)
    res_dtype = result_dtype(c, out_f32)
    st = 2.0 ** -8 if res_dtype is BF16 else 0.0
    ratio = lambda got: worst_ratio(got, ref, bsum, st)

    honest32 = conv_cpu(c, a.float(), b.float())
    r = ratio(store(honest32, res_dtype))
    print(f"{name} {'f32' if res_dtype is FP32 else 'bf16'} out: "
          f"honest fp32 = {r:.4f}")
    assert r <= 1.0, f"{name}: honest fp32 arithmetic is {r:.3f} x the bound"

    mutants = {}
    # one padding tap at one border pixel reads the neighbouring pixel
    # instead of zero
    pad_tap = first_tap(c, want_padding=True)
    if pad_tap is not None:
        idx, term = tap_term(c, a, b, pad_tap, slice(None))
        m = ref.clone()
        m[idx] += term
        mutants["padding tap reads its neighbour"] = store(m, res_dtype)
    # one 8-channel slot of one tap dropped, at one pixel
    idx, term = tap_term(c, a, b, first_tap(c, want_padding=False),
                         contracted_slot(c))
    m = ref.clone()
    m[idx] -= term
    mutants["8-channel slot of one tap dropped"] = store(m, res_dtype)
    # result shifted by one pixel (wgrad: by one tap)
    if ref.shape[2] > 1:
        mutants["shifted by one pixel"] = store(torch.roll(ref, 1, 2),
                                                res_dtype)
    if res_dtype is BF16:
        mutants["truncating bf16 store"] = truncate_bf16(honest32)
    if c["dtype"] is FP32:
        narrow = conv_cpu(c, a.to(BF16).float(), b.to(BF16).float())
        mutants["operands narrowed to bf16"] = store(narrow, res_dtype)
    assert len(mutants) >= 2
    for what, got in mutants.items():
        r = ratio(got)
        print(f"{name}: {what} = {r:.3f}")
        assert r > 1.0, f"{name}: '{what}' passes the bound ({r:.3f})"

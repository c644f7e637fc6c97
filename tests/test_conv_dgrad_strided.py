"""Strided conv dgrad through ``conv_dgrad`` against a float64 reference
(``torch.nn.grad.conv2d_input`` on the CPU).

Products of bf16 values are exact in fp32, so the only error of the kernel is
fp32 summation in some order, elementwise

    |got - ref| <= KH * KW * Cout * 2^-23 * conv2d_input(|dy|, |w|)

(the (n-1) u sum|t_i| bound with u = 2^-24, doubled for MFMA-internal
rounding; the same bound covers the rounded products of the fp32 kernel),
plus 2^-8 relative for the one rounding of a bf16 store. Factor 1, no free
constants: the form tests/test_conv_wgrad_px.py uses.

Stride 2 with Cout % 32 == 0 takes the phase-decomposed kernel
(csrc/dgrad_phase_map.h); the last two cases stay on the generic one. The
XCD remap of the block ids needs more than 200 MiB of activations besides 64
blocks, so no case here switches it on; tests/test_dgrad_phase_map.py checks
it on the CPU."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"

# (N, H, W, Cin, Cout, K, stride, pad)
CASES = {
    # narrow (128 x 64) tile; 32 rows per class, several classes per tile range
    "narrow_tile": (2, 8, 8, 64, 128, 3, 2, 1),
    # wide (128 x 128) tile
    "wide_tile": (2, 8, 8, 128, 256, 3, 2, 1),
    # 27 rows per class: every class tile partial; one k-step per tap
    "partial_tiles_one_kstep": (3, 6, 6, 64, 32, 3, 2, 1),
    # odd extents: unequal classes, ho / wo bounds bite; 3 k-steps per tap
    "odd_extents": (1, 5, 7, 64, 96, 3, 2, 1),
    # 1x1: three classes without taps must come out as exact zeros
    "empty_classes": (2, 8, 8, 64, 128, 1, 2, 0),
    # 640 rows per class: five full tiles each, 20 blocks (many blocks per
    # class; still below the remap's thresholds, see above)
    "many_tiles": (40, 8, 8, 128, 64, 3, 2, 1),
    # Cout not a multiple of 32: generic kernel
    "cout_48_generic": (2, 8, 8, 64, 48, 3, 2, 1),
    # stride 3: generic kernel
    "stride_3_generic": (2, 9, 9, 64, 64, 3, 3, 1),
}
FP32_CASES = ["narrow_tile", "wide_tile"]


@functools.lru_cache(maxsize=None)
def problem(name):
    """bf16-valued inputs, float64 reference and summation bound on the CPU;
    computed once per case and never modified."""
    N, H, W, Cin, Cout, K, s, p = CASES[name]
    HO, WO = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    g = torch.Generator().manual_seed(4321 + sum(CASES[name]))
    dy = torch.randn(N, HO, WO, Cout, generator=g).to(torch.bfloat16)
    w = torch.randn(Cout, K, K, Cin, generator=g).mul(0.1).to(torch.bfloat16)
    dyn = dy.double().permute(0, 3, 1, 2)
    wn = w.double().permute(0, 3, 1, 2)
    shape = (N, Cin, H, W)
    ref = torch.nn.grad.conv2d_input(shape, wn, dyn, stride=s, padding=p)
    mag = torch.nn.grad.conv2d_input(shape, wn.abs(), dyn.abs(), stride=s,
                                     padding=p)
    bound = K * K * Cout * 2.0 ** -23 * mag
    to_nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return dy, w, to_nhwc(ref), to_nhwc(bound)


def run(name, dtype):
    N, H, W, Cin, Cout, K, s, p = CASES[name]
    dy, w, ref, bound = problem(name)
    dy_d = dy.to(DEV, dtype).contiguous()
    w_d = w.to(DEV, dtype).contiguous()
    if name == "empty_classes":
        # a block of the output's size, full of NaN, goes back to the
        # allocator just before the call: a row the kernel skips shows
        junk = torch.full((N, H, W, Cin), float("nan"), dtype=dtype, device=DEV)
        del junk
    dx = OPS.conv_dgrad(dy_d, w_d, H, W, s, p)
    assert dx.dtype == dtype and tuple(dx.shape) == (N, H, W, Cin)
    return dx.cpu(), ref, bound


def check(tag, name, dx, ref, bound, store_rel):
    assert torch.isfinite(dx).all(), f"{name}: non-finite dx"
    err = (dx.double() - ref).abs()
    lim = bound + store_rel * ref.abs()
    # a pixel no tap reaches has ref == bound == 0 and must be exactly 0
    ratio = torch.where(lim > 0, err / lim, (err > 0).double() * 2).max().item()
    print(f"dgrad {tag} {name} {CASES[name]}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error is {ratio:.3f} x the bound"


@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_bf16(name):
    dx, ref, bound = run(name, torch.bfloat16)
    check("bf16", name, dx, ref, bound, 2.0 ** -8)
    if name == "empty_classes":
        assert (dx[:, 1::2] == 0).all() and (dx[:, :, 1::2] == 0).all()


@pytest.mark.parametrize("name", FP32_CASES)
def test_dgrad_fp32(name):
    dx, ref, bound = run(name, torch.float32)
    check("fp32", name, dx, ref, bound, 0.0)

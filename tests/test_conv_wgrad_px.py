"""3x3 stride-1 wgrad through ``conv_wgrad`` against a float64 reference,
with a bound tight enough to see a wrong halo.

Products of bf16 values are exact in fp32, so the only error of the kernel is
fp32 summation in some order: elementwise

    |got - ref| <= npix * 2^-23 * conv2d_weight(|x|, |dy|)

which is the standard (n-1) u sum|t_i| bound with u = 2^-24, doubled for
MFMA-internal rounding and atomic order. (The 0.06 sqrt(npix) bound of
test_kernels_gpu.py passes a missing zero border, which moves an element by
about 0.1 sqrt(npix / 16).)

Shapes are the smallest that reach each way of going wrong; see CASES."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"

# (N, H, W, Cin, Cout)
CASES = {
    # one k-step that spans two images; prologue and tail with nothing in flight
    "two_images_one_step": (2, 4, 4, 64, 64),
    # three steps, two ci tiles
    "three_steps_two_ci": (6, 4, 4, 128, 64),
    # four image rows per step, two co tiles
    "four_rows_two_co": (2, 8, 8, 64, 128),
    # N = 1: top and bottom halo in every image
    "single_image": (1, 16, 16, 64, 64),
    # one row per step, three co tiles
    "row_per_step_three_co": (1, 32, 32, 64, 192),
    # odd N
    "odd_n": (3, 32, 32, 64, 64),
    # non-square, accepted by the gate (two 16-wide rows per step, H % 2 == 0)
    "non_square": (2, 8, 16, 64, 64),
    # W = 12 does not divide 32: generic kernel, fed the relocated transpose
    "outside_gate_w12": (2, 12, 12, 64, 64),
    # short last split. 8 x 8 = 64 tiles -> target 512 / 64 = 8 splits; 18
    # images of 4x4 are 288 pixels = 9 k-steps > 8, so steps per split =
    # ceil(9 / 8) = 2 and the grid has ceil(9 / 2) = 5 slices, the last with
    # a single step
    "short_last_split": (18, 4, 4, 512, 512),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """bf16 inputs on the GPU, float64 reference and error bound on the CPU;
    computed once per case and never modified."""
    N, H, W, Cin, Cout = CASES[name]
    g = torch.Generator().manual_seed(1234 + sum(CASES[name]))
    x = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16)
    dy = torch.randn(N, H, W, Cout, generator=g).mul(0.1).to(torch.bfloat16)
    xn = x.double().permute(0, 3, 1, 2)
    dyn = dy.double().permute(0, 3, 1, 2)
    shape = (Cout, Cin, 3, 3)
    ref = torch.nn.grad.conv2d_weight(xn, shape, dyn, stride=1, padding=1)
    mag = torch.nn.grad.conv2d_weight(xn.abs(), shape, dyn.abs(), stride=1,
                                      padding=1)
    npix = N * H * W
    bound = npix * 2.0 ** -23 * mag
    to_ohwi = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return (x.to(DEV).contiguous(), dy.to(DEV).contiguous(), to_ohwi(ref),
            to_ohwi(bound))


def worst_ratio(got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    return (err / bound).max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_fp32_out(name):
    x, dy, ref, bound = problem(name)
    dw = OPS.conv_wgrad(dy, x, 3, 3, 1, 1, True)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == tuple(ref.shape)
    ratio = worst_ratio(dw, ref, bound)
    print(f"wgrad {name} {CASES[name]}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: error is {ratio:.3f} x the fp32 summation bound"


def test_wgrad_bf16_out():
    name = "four_rows_two_co"
    x, dy, ref, bound = problem(name)
    dw = OPS.conv_wgrad(dy, x, 3, 3, 1, 1, False)
    assert dw.dtype == torch.bfloat16
    # one rounding of the fp32 result to bf16 on top of the summation bound
    err = (dw.double().cpu() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + bound
    ratio = (err / lim).max().item()
    print(f"wgrad bf16 out {CASES[name]}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_routes():
    """The gate takes every accepted case above and rejects W = 12."""
    for name, (N, H, W, Cin, Cout) in CASES.items():
        el = OPS.wgrad_px_eligible(True, N, H, W, Cin, Cout, 3, 3, 1, 1)
        assert el == (name != "outside_gate_w12"), name
    steps, per_split, splits = OPS.wgrad_px_split(18, 4, 4, 512, 512)
    assert (steps, per_split, splits) == (9, 2, 5)

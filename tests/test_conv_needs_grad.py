"""``Conv2dFn.backward`` computes only the gradients somebody asked for: the
stem's input is the data batch, and its dx used to be computed and dropped.

Shape: the stem in small (Cin = 3, 3x3 stride 1 pad 1). References are
float64 on the CPU; bounds are the fp32 summation bounds of
tests/test_conv_wgrad_px.py and tests/test_conv_dgrad_strided.py plus 2^-8
relative for a bf16 store."""

import functools

import pytest
import torch

from baton_amd.ops import functional as BF

N, H, W, CIN, COUT, K, STRIDE, PAD = 4, 8, 8, 3, 64, 3, 1, 1


@functools.lru_cache(maxsize=None)
def problem():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, H, W, CIN, generator=g).to(torch.bfloat16)
    w = torch.randn(COUT, K, K, CIN, generator=g).mul(0.1).to(torch.bfloat16)
    dy = torch.randn(N, H, W, COUT, generator=g).mul(0.1).to(torch.bfloat16)
    xn, wn, dyn = (t.double().permute(0, 3, 1, 2) for t in (x, w, dy))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    kw = dict(stride=STRIDE, padding=PAD)
    dw = torch.nn.grad.conv2d_weight(xn, wn.shape, dyn, **kw)
    dw_mag = torch.nn.grad.conv2d_weight(xn.abs(), wn.shape, dyn.abs(), **kw)
    dx = torch.nn.grad.conv2d_input(xn.shape, wn, dyn, **kw)
    dx_mag = torch.nn.grad.conv2d_input(xn.shape, wn.abs(), dyn.abs(), **kw)
    return dict(x=x, w=w, dy=dy,
                dw=nhwc(dw), dw_bound=N * H * W * 2.0 ** -23 * nhwc(dw_mag),
                dx=nhwc(dx), dx_bound=K * K * COUT * 2.0 ** -23 * nhwc(dx_mag))


def backward(dev, dtype, x_requires_grad):
    p = problem()
    x = p["x"].to(dev, dtype).requires_grad_(x_requires_grad)
    w = p["w"].to(dev, dtype).requires_grad_(True)
    y = BF.conv2d(x, w, STRIDE, PAD)
    y.backward(p["dy"].to(dev, dtype))
    return x.grad, w.grad


def close(got, ref, bound, store_rel):
    err = (got.double().cpu() - ref).abs()
    return (err / (bound + store_rel * ref.abs())).max().item() <= 1.0


def boom(*a, **k):
    raise AssertionError("dgrad was called for an input that needs no grad")


def test_cpu_no_dx_when_not_needed(monkeypatch):
    p = problem()           # the reference itself uses conv2d_input
    monkeypatch.setattr(torch.nn.grad, "conv2d_input", boom)
    dx, dw = backward("cpu", torch.float32, False)
    assert dx is None
    assert close(dw, p["dw"], p["dw_bound"], 0.0)


def test_cpu_both_when_needed():
    p = problem()
    dx, dw = backward("cpu", torch.float32, True)
    assert close(dx, p["dx"], p["dx_bound"], 0.0)
    assert close(dw, p["dw"], p["dw_bound"], 0.0)


@pytest.mark.gpu
def test_gpu_no_dx_when_not_needed(monkeypatch):
    from baton_amd.ops._ext import require_hip

    p = problem()
    monkeypatch.setattr(require_hip(), "conv_dgrad", boom)
    dx, dw = backward("cuda:0", torch.bfloat16, False)
    assert dx is None
    assert dw.dtype == torch.bfloat16
    assert close(dw, p["dw"], p["dw_bound"], 2.0 ** -8)


@pytest.mark.gpu
def test_gpu_both_when_needed():
    p = problem()
    dx, dw = backward("cuda:0", torch.bfloat16, True)
    assert close(dx, p["dx"], p["dx_bound"], 2.0 ** -8)
    assert close(dw, p["dw"], p["dw_bound"], 2.0 ** -8)

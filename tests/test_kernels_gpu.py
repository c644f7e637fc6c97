"""GPU kernel numerics: every HIP kernel vs a plain torch fp32 reference
(SURVEY.md §4 kernel unit tests). Run via gpurun:
    python -m pytest tests/test_kernels_gpu.py -m gpu -x -q

Transpose-detecting by construction: all operands are asymmetric random
tensors (guide §5.4 rule 16)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"


def assert_close(got, ref, rtol, atol, msg=""):
    got = got.float()
    ref = ref.float()
    err = (got - ref).abs()
    denom = ref.abs().clamp_min(1.0)
    rel = (err / denom).max().item()
    assert err.max().item() < atol or rel < rtol, (
        f"{msg}: max abs err {err.max().item():.4e}, max rel {rel:.4e}"
    )


# ---- GEMM ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize(
    "M,N,K", [(128, 128, 64), (256, 512, 128), (100, 70, 50), (33, 257, 129)]
)
def test_gemm_nt(dtype, M, N, K):
    torch.manual_seed(0)
    A = torch.randn(M, K, device=DEV).to(dtype).contiguous()
    B = torch.randn(N, K, device=DEV).to(dtype).contiguous()
    C = OPS.gemm(A, B, 0)
    ref = A.float() @ B.float().t()
    tol = 1e-4 if dtype == torch.float32 else 0.05
    assert_close(C, ref, tol, tol * K**0.5, f"gemm NT {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (100, 70, 50)])
def test_gemm_nn(dtype, M, N, K):
    torch.manual_seed(1)
    A = torch.randn(M, K, device=DEV).to(dtype).contiguous()
    B = torch.randn(K, N, device=DEV).to(dtype).contiguous()
    C = OPS.gemm(A, B, 1)
    ref = A.float() @ B.float()
    tol = 1e-4 if dtype == torch.float32 else 0.05
    assert_close(C, ref, tol, tol * K**0.5, f"gemm NN {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (70, 100, 60)])
def test_gemm_tn(dtype, M, N, K):
    torch.manual_seed(2)
    A = torch.randn(K, M, device=DEV).to(dtype).contiguous()
    B = torch.randn(K, N, device=DEV).to(dtype).contiguous()
    C = OPS.gemm(A, B, 2)
    ref = A.float().t() @ B.float()
    tol = 1e-4 if dtype == torch.float32 else 0.05
    assert_close(C, ref, tol, tol * K**0.5, f"gemm TN {dtype}")


def test_gemm_bias_relu():
    torch.manual_seed(3)
    A = torch.randn(64, 32, device=DEV, dtype=torch.bfloat16).contiguous()
    B = torch.randn(48, 32, device=DEV, dtype=torch.bfloat16).contiguous()
    bias = torch.randn(48, device=DEV, dtype=torch.float32)
    C = OPS.gemm(A, B, 0, bias, True, False, 1.0, 0.0)
    ref = (A.float() @ B.float().t() + bias).clamp_min(0)
    assert_close(C, ref, 0.05, 0.3, "gemm bias+relu")
    assert (C.float() >= 0).all()


def test_gemm_wgrad_f32_out():
    torch.manual_seed(4)
    A = torch.randn(64, 128, device=DEV, dtype=torch.bfloat16).contiguous()
    B = torch.randn(64, 96, device=DEV, dtype=torch.bfloat16).contiguous()
    C = OPS.gemm(A, B, 2, torch.Tensor(), False, True, 1.0, 0.0)
    assert C.dtype == torch.float32
    ref = A.float().t() @ B.float()
    assert_close(C, ref, 0.05, 0.5, "gemm TN f32-out")


# ---- conv ------------------------------------------------------------------

def _conv_ref(x, w, stride, pad):
    # NHWC tensors -> torch NCHW fp32 reference
    xn = x.float().permute(0, 3, 1, 2)
    wn = w.float().permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xn, wn, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


CONV_CASES = [
    # N, H, W, Cin, Cout, K, stride, pad      — covers stem (Cin=3), fast
    # path (Cin%32==0), stride-2, and 1x1 downsample
    (4, 32, 32, 3, 64, 3, 1, 1),
    (4, 16, 16, 64, 64, 3, 1, 1),
    (4, 16, 16, 64, 128, 3, 2, 1),
    (4, 16, 16, 64, 128, 1, 2, 0),
    (2, 8, 8, 128, 256, 3, 1, 1),
    # tap-replicated wgrad path edges: one 32-px k-step spanning two
    # images (W=4), and the W=32 single-row-advance case
    (4, 4, 4, 128, 64, 3, 1, 1),
    (3, 32, 32, 64, 64, 3, 1, 1),
    # 1x1 stride-1: wgrad routes through the split-K NN GEMM
    (4, 16, 16, 128, 256, 1, 1, 0),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd(dtype, case):
    N, H, W, Cin, Cout, K, s, p = case
    torch.manual_seed(5)
    x = torch.randn(N, H, W, Cin, device=DEV).to(dtype).contiguous()
    w = torch.randn(Cout, K, K, Cin, device=DEV).to(dtype).mul(0.1).contiguous()
    y = OPS.conv_fwd(x, w, s, p)
    ref = _conv_ref(x, w, s, p)
    tol = 1e-4 if dtype == torch.float32 else 0.06
    assert_close(y, ref, tol, tol * (Cin * K * K) ** 0.5, f"conv fwd {case}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_dgrad(dtype, case):
    N, H, W, Cin, Cout, K, s, p = case
    torch.manual_seed(6)
    HO = (H + 2 * p - K) // s + 1
    WO = (W + 2 * p - K) // s + 1
    dy = torch.randn(N, HO, WO, Cout, device=DEV).to(dtype).contiguous()
    w = torch.randn(Cout, K, K, Cin, device=DEV).to(dtype).mul(0.1).contiguous()
    dx = OPS.conv_dgrad(dy, w, H, W, s, p)
    dyn = dy.float().permute(0, 3, 1, 2)
    wn = w.float().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), wn, dyn, stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    tol = 1e-4 if dtype == torch.float32 else 0.06
    assert_close(dx, ref, tol, tol * (Cout * K * K) ** 0.5, f"conv dgrad {case}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_wgrad(dtype, case):
    N, H, W, Cin, Cout, K, s, p = case
    torch.manual_seed(7)
    HO = (H + 2 * p - K) // s + 1
    WO = (W + 2 * p - K) // s + 1
    x = torch.randn(N, H, W, Cin, device=DEV).to(dtype).contiguous()
    dy = torch.randn(N, HO, WO, Cout, device=DEV).to(dtype).mul(0.1).contiguous()
    dw = OPS.conv_wgrad(dy, x, K, K, s, p, True)  # fp32 out
    xn = x.float().permute(0, 3, 1, 2)
    dyn = dy.float().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, K, K), dyn, stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    tol = 1e-4 if dtype == torch.float32 else 0.06
    npix = N * HO * WO
    assert_close(dw, ref, tol, tol * npix**0.5, f"conv wgrad {case}")


# ---- layernorm -------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,C", [(64, 768), (33, 100), (256, 1024)])
def test_layernorm(dtype, R, C):
    torch.manual_seed(8)
    x = torch.randn(R, C, device=DEV).to(dtype).contiguous()
    w = (torch.randn(C, device=DEV) * 0.5 + 1).to(dtype).contiguous()
    b = torch.randn(C, device=DEV).to(dtype).contiguous()
    y, mean, rstd = OPS.ln_fwd(x, w, b, 1e-5)
    xf = x.float()
    mu = xf.mean(1, keepdim=True)
    var = xf.var(1, unbiased=False, keepdim=True)
    ref = (xf - mu) * (var + 1e-5).rsqrt() * w.float() + b.float()
    tol = 1e-4 if dtype == torch.float32 else 0.03
    assert_close(y, ref, tol, tol, "ln fwd")

    dy = torch.randn(R, C, device=DEV).to(dtype).contiguous()
    dx, dw, db = OPS.ln_bwd(x, dy, w, mean, rstd)
    xr = x.float().detach().requires_grad_(True)
    wr = w.float().detach().requires_grad_(True)
    br = b.float().detach().requires_grad_(True)
    mu = xr.mean(1, keepdim=True)
    var = ((xr - mu) ** 2).mean(1, keepdim=True)
    yr = (xr - mu) * (var + 1e-5).rsqrt() * wr + br
    yr.backward(dy.float())
    tol = 1e-3 if dtype == torch.float32 else 0.05
    assert_close(dx, xr.grad, tol, tol, "ln dx")
    assert_close(dw, wr.grad, tol, tol * R**0.5, "ln dw")
    assert_close(db, br.grad, tol, tol * R**0.5, "ln db")


# ---- batchnorm -------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_train(dtype, relu):
    torch.manual_seed(9)
    M, C = 512, 64
    x = torch.randn(M, C, device=DEV).to(dtype).contiguous()
    gamma = (torch.randn(C, device=DEV) * 0.3 + 1).float()
    beta = torch.randn(C, device=DEV).float()
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    y, mean, rstd = OPS.bn_fwd_train(x, gamma, beta, rm, rv, 0.1, 1e-5, relu)

    xf = x.float()
    mu = xf.mean(0)
    var = xf.var(0, unbiased=False)
    ref = (xf - mu) * (var + 1e-5).rsqrt() * gamma + beta
    if relu:
        ref = ref.clamp_min(0)
    tol = 1e-4 if dtype == torch.float32 else 0.03
    assert_close(y, ref, tol, tol, "bn fwd")
    # running stats
    assert_close(rm, 0.1 * mu, 1e-3, 1e-4, "bn running_mean")
    assert_close(rv, 0.9 + 0.1 * xf.var(0, unbiased=True), 1e-3, 1e-3, "bn running_var")

    dy = torch.randn(M, C, device=DEV).to(dtype).contiguous()
    dx, dgamma, dbeta = OPS.bn_bwd(x, dy, y, mean, rstd, gamma, relu)
    xr = xf.detach().requires_grad_(True)
    gr = gamma.detach().requires_grad_(True)
    br = beta.detach().requires_grad_(True)
    mu = xr.mean(0)
    var = ((xr - mu) ** 2).mean(0)
    yr = (xr - mu) * (var + 1e-5).rsqrt() * gr + br
    if relu:
        yr = yr.clamp_min(0)
    yr.backward(dy.float())
    tol = 1e-3 if dtype == torch.float32 else 0.05
    assert_close(dx, xr.grad, tol, tol, "bn dx")
    assert_close(dgamma, gr.grad, tol, tol * M**0.5, "bn dgamma")
    assert_close(dbeta, br.grad, tol, tol * M**0.5, "bn dbeta")


# ---- losses ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mse(dtype):
    torch.manual_seed(10)
    x = torch.randn(1000, device=DEV).to(dtype).contiguous()
    y = torch.randn(1000, device=DEV).to(dtype).contiguous()
    loss = OPS.mse_fwd(x, y)
    ref = torch.nn.functional.mse_loss(x.float(), y.float())
    assert_close(loss, ref, 1e-3 if dtype == torch.float32 else 0.02, 1e-3, "mse")
    dout = torch.tensor(1.7, device=DEV)
    dx = OPS.mse_bwd(x, y, dout)
    ref_dx = 2 * (x.float() - y.float()) / x.numel() * 1.7
    assert_close(dx, ref_dx, 0.02, 1e-4, "mse bwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(64, 10), (32, 1000), (8, 30522)])
def test_cross_entropy(dtype, B, C):
    torch.manual_seed(11)
    logits = torch.randn(B, C, device=DEV).to(dtype).mul(2).contiguous()
    target = torch.randint(0, C, (B,), device=DEV)
    loss, lse = OPS.ce_fwd(logits, target)
    ref = torch.nn.functional.cross_entropy(logits.float(), target)
    tol = 1e-4 if dtype == torch.float32 else 0.02
    assert_close(loss, ref, tol, tol, "ce loss")
    dout = torch.tensor(1.0, device=DEV)
    dx = OPS.ce_bwd(logits, target, lse, dout)
    lr = logits.float().detach().requires_grad_(True)
    torch.nn.functional.cross_entropy(lr, target).backward()
    assert_close(dx, lr.grad, 0.03, 1e-4, "ce bwd")


# ---- elementwise -----------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu_add_gelu(dtype):
    torch.manual_seed(12)
    x = torch.randn(3333, device=DEV).to(dtype).contiguous()
    b = torch.randn(3333, device=DEV).to(dtype).contiguous()
    assert_close(OPS.relu_fwd(x), x.float().clamp_min(0), 1e-6, 1e-6, "relu")
    y = OPS.add_relu_fwd(x, b)
    assert_close(y, (x.float() + b.float()).clamp_min(0), 0.02, 0.02, "add_relu")
    dy = torch.randn(3333, device=DEV).to(dtype).contiguous()
    dx = OPS.relu_bwd(dy, y)
    assert_close(dx, dy.float() * (y.float() > 0), 1e-6, 1e-6, "relu bwd")
    g = OPS.gelu_fwd(x)
    ref = torch.nn.functional.gelu(x.float(), approximate="tanh")
    assert_close(g, ref, 0.02, 0.02, "gelu")
    dg = OPS.gelu_bwd(dy, x)
    xr = x.float().detach().requires_grad_(True)
    torch.nn.functional.gelu(xr, approximate="tanh").backward(dy.float())
    assert_close(dg, xr.grad, 0.03, 0.03, "gelu bwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add_scaled_and_scale(dtype):
    torch.manual_seed(21)
    a = torch.randn(4099, device=DEV).to(dtype).contiguous()
    b = torch.randn(4099, device=DEV).to(dtype).contiguous()
    z = OPS.add_scaled_fwd(a, b, 0.125)
    assert_close(z, a.float() + 0.125 * b.float(), 0.02, 0.02, "add_scaled")
    s = OPS.scale_fwd(b, -1.5)
    assert_close(s, -1.5 * b.float(), 0.02, 0.02, "scale")


def test_lora_linear_fused_join_gpu():
    """lora_linear (combine fused into the rank-r B GEMM's beta=1
    C-accumulate epilogue, in place) vs an fp32 composition: forward and
    the lora_a / lora_b / x grads at a llama-like shape."""
    torch.manual_seed(22)
    B, S, K, r, N = 2, 256, 512, 16, 768
    x = (torch.randn(B, S, K, device=DEV) * 0.5).bfloat16().requires_grad_(True)
    w = (torch.randn(N, K, device=DEV) * 0.05).bfloat16()
    a = (torch.randn(r, K, device=DEV) * 0.05).bfloat16().requires_grad_(True)
    b = (torch.randn(N, r, device=DEV) * 0.05).bfloat16().requires_grad_(True)
    scaling = 2.0
    from baton_amd.ops import functional as BF

    y = BF.lora_linear(x, w, a, b, scaling)
    dz = (torch.randn_like(y) * 0.1).bfloat16()
    y.backward(dz)

    xr = x.detach().float().requires_grad_(True)
    ar = a.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    yr = xr @ w.float().t() + scaling * ((xr @ ar.t()) @ br.t())
    yr.backward(dz.float())
    assert_close(y, yr, 0.05, 0.06 * K**0.5, "lora fused fwd")
    assert_close(x.grad, xr.grad, 0.05, 0.06 * N**0.5, "lora dx")
    assert_close(a.grad, ar.grad, 0.05, 0.06 * (B * S) ** 0.5, "lora dA")
    assert_close(b.grad, br.grad, 0.05, 0.06 * (B * S) ** 0.5, "lora dB")


@pytest.mark.parametrize("packed,causal,kvh", [(True, False, 4), (False, True, 2), (False, False, 4)])
def test_attention_strided_vs_torch(packed, causal, kvh):
    """Strided-view attention (no permute copies) vs a torch fp32
    reference, fwd + bwd, incl. packed QKV and GQA."""
    import baton_amd.ops.functional as BF
    torch.manual_seed(33)
    B, S, h, dh = 3, 64, 4, 32
    if packed:
        qkv = (torch.randn(B, S, 3, h, dh, device=DEV).bfloat16() * 0.5
               ).requires_grad_(True)
        o = BF.attention_qkv(qkv, causal=causal)
        q, k, v = (qkv.float()[:, :, i] for i in range(3))
    else:
        q_t = (torch.randn(B, S, h, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
        k_t = (torch.randn(B, S, kvh, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
        v_t = (torch.randn(B, S, kvh, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
        o = BF.attention_bshd(q_t, k_t, v_t, causal=causal)
        g = h // kvh
        q = q_t.float()
        k = k_t.float().repeat_interleave(g, dim=2)
        v = v_t.float().repeat_interleave(g, dim=2)
    # torch reference in fp32, [B,h,S,dh]
    qr = q.detach().permute(0, 2, 1, 3).requires_grad_(True)
    kr = k.detach().permute(0, 2, 1, 3).requires_grad_(True)
    vr = v.detach().permute(0, 2, 1, 3).requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        qr, kr, vr, is_causal=causal)
    ref_o = ref.permute(0, 2, 1, 3)
    assert_close(o, ref_o, 0.03, 0.03, "attn fwd")
    do = torch.randn_like(ref_o)
    ref_o.backward(do)
    o.backward(do.to(o.dtype))
    if packed:
        dq_ref = qr.grad.permute(0, 2, 1, 3)
        dk_ref = kr.grad.permute(0, 2, 1, 3)
        dv_ref = vr.grad.permute(0, 2, 1, 3)
        assert_close(qkv.grad[:, :, 0], dq_ref, 0.05, 0.05, "attn dq")
        assert_close(qkv.grad[:, :, 1], dk_ref, 0.05, 0.05, "attn dk")
        assert_close(qkv.grad[:, :, 2], dv_ref, 0.05, 0.05, "attn dv")
    else:
        g = h // kvh
        dq_ref = qr.grad.permute(0, 2, 1, 3)
        dk_ref = kr.grad.permute(0, 2, 1, 3).view(B, S, kvh, g, dh).sum(3)
        dv_ref = vr.grad.permute(0, 2, 1, 3).view(B, S, kvh, g, dh).sum(3)
        assert_close(q_t.grad, dq_ref, 0.05, 0.05, "attn dq")
        assert_close(k_t.grad, dk_ref, 0.05, 0.08, "attn dk")
        assert_close(v_t.grad, dv_ref, 0.05, 0.08, "attn dv")


# ---- optimizers ------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_sgd_matches_torch(dtype):
    torch.manual_seed(13)
    n = 10007
    p0 = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    # torch reference in fp32
    pref = p0.clone().requires_grad_(False)
    mref = torch.zeros(n, device=DEV)
    lr, mom, wd = 0.01, 0.9, 1e-4
    for _ in range(3):
        gr = g + wd * pref
        mref = mom * mref + gr
        pref = pref - lr * mref
    p = p0.to(dtype).contiguous()
    m = torch.zeros(n, device=DEV)
    for _ in range(3):
        OPS.sgd_step(p, g.to(dtype), m, lr, mom, wd)
    tol = 1e-5 if dtype == torch.float32 else 0.03
    assert_close(p, pref, tol, tol, "sgd trajectory")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_adam_matches_torch(dtype):
    torch.manual_seed(14)
    n = 4097
    p0 = torch.randn(n, device=DEV)
    param_ref = torch.nn.Parameter(p0.clone())
    opt_ref = torch.optim.Adam([param_ref], lr=0.01, weight_decay=1e-3)
    g = torch.randn(n, device=DEV)

    p = p0.to(dtype).contiguous()
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t in range(1, 4):
        param_ref.grad = g.clone()
        opt_ref.step()
        bc1 = 1 - b1**t
        bc2 = 1 - b2**t
        OPS.adam_step(p, g.to(dtype), m, v, 0.01, b1, b2, eps, 1e-3, bc1, bc2)
    tol = 1e-4 if dtype == torch.float32 else 0.03
    assert_close(p, param_ref.detach(), tol, tol, "adam trajectory")


# ---- fedmath ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scale_cast_roundtrip(dtype):
    torch.manual_seed(15)
    src = torch.randn(5001, device=DEV).to(dtype).contiguous()
    dst = torch.empty(5001, device=DEV, dtype=torch.float32)
    OPS.scale_cast(dst, src, 0.25)
    assert_close(dst, src.float() * 0.25, 1e-6, 1e-6, "scale_cast")
    back = torch.empty_like(src)
    OPS.cast_copy(back, dst)
    assert_close(back, (src.float() * 0.25), 0.01, 0.01, "cast_copy")


def test_axpby():
    torch.manual_seed(16)
    y = torch.randn(777, device=DEV)
    x = torch.randn(777, device=DEV)
    y0 = y.clone()
    OPS.axpby(y, x, 2.0, 0.5)
    assert_close(y, 2.0 * x + 0.5 * y0, 1e-6, 1e-6, "axpby")


# ---- end-to-end ------------------------------------------------------------

def test_resnet18_step_bf16():
    """One full federated-client step of the flagship model through the HIP
    path; checks finiteness and that a step changes the params."""
    from baton_amd.models.resnet import make_synthetic_cifar, resnet18
    from baton_amd.ops import functional as BF
    from baton_amd.ops.optim import FusedSGD

    torch.manual_seed(17)
    model = resnet18().to(DEV).to(torch.bfloat16)
    x, y = make_synthetic_cifar(16, dtype=torch.bfloat16)
    x, y = x.to(DEV), y.to(DEV)
    opt = FusedSGD(model.parameters(), lr=1e-2)
    before = model.fc.weight.detach().clone()
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = BF.cross_entropy(model(x).contiguous(), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses), f"NaN loss {losses}"
    assert not torch.equal(before, model.fc.weight.detach())
    # training on one batch must reduce loss
    assert losses[-1] < losses[0] + 0.5, f"diverging: {losses}"


def test_hip_graph_step_matches_eager():
    """GraphedTrainStep (hipGraph capture) must track the eager step: same
    model/data/seed, losses within bf16+atomic-nondeterminism tolerance."""
    from baton_amd.models.resnet import make_synthetic_cifar, resnet18
    from baton_amd.ops import functional as BF
    from baton_amd.ops.optim import FusedSGD
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.runtime.graph import GraphedTrainStep

    def run(graphed: bool):
        torch.manual_seed(42)
        model = resnet18().to(DEV).to(torch.bfloat16)
        model.train()
        arena = FlatParamArena(model)
        opt = FusedSGD.from_arena(arena, lr=1e-2)
        x, y = make_synthetic_cifar(64, dtype=torch.bfloat16)
        x, y = x.to(DEV), y.to(DEV)
        loss_fn = lambda lg, t: BF.cross_entropy(lg.contiguous(), t)
        losses = []
        if graphed:
            step = GraphedTrainStep(model, opt, loss_fn, x[:32], y[:32],
                                    warmup_steps=0)
            for _ in range(4):
                l = step(x[:32], y[:32])
                losses.append(float(l.item()))
        else:
            for _ in range(4):
                opt.zero_grad()
                l = loss_fn(model(x[:32]), y[:32])
                l.backward()
                opt.step()
                losses.append(float(l.item()))
        return losses

    eager = run(False)
    graphed = run(True)
    assert all(v == v for v in graphed), f"NaN in graphed losses {graphed}"
    for a, b in zip(eager, graphed):
        assert abs(a - b) < 0.2, f"graph vs eager diverged: {eager} vs {graphed}"


# ---- transformer kernels ---------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gemm_batched(dtype, layout):
    torch.manual_seed(20)
    nb, M, N, K = 6, 128, 64, 96
    if layout == 0:
        A = torch.randn(nb, M, K, device=DEV).to(dtype)
        B = torch.randn(nb, N, K, device=DEV).to(dtype)
        ref = torch.bmm(A.float(), B.float().transpose(1, 2))
    elif layout == 1:
        A = torch.randn(nb, M, K, device=DEV).to(dtype)
        B = torch.randn(nb, K, N, device=DEV).to(dtype)
        ref = torch.bmm(A.float(), B.float())
    else:
        A = torch.randn(nb, K, M, device=DEV).to(dtype)
        B = torch.randn(nb, K, N, device=DEV).to(dtype)
        ref = torch.bmm(A.float().transpose(1, 2), B.float())
    C = OPS.gemm_batched(A.contiguous(), B.contiguous(), layout)
    tol = 1e-4 if dtype == torch.float32 else 0.05
    assert_close(C, ref, tol, tol * K**0.5, f"gemm_batched l{layout}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("causal", [0, 64])
def test_softmax_kernel(dtype, causal):
    torch.manual_seed(21)
    R, C = 256, 64
    x = torch.randn(R, C, device=DEV).to(dtype).mul(3).contiguous()
    scale = 0.125
    y = OPS.softmax_fwd(x, scale, causal)
    z = x.float() * scale
    if causal:
        q = torch.arange(R, device=DEV) % causal
        mask = torch.arange(C, device=DEV)[None, :] > q[:, None]
        z = z.masked_fill(mask, float("-inf"))
    ref = torch.softmax(z, dim=-1)
    tol = 1e-5 if dtype == torch.float32 else 0.02
    assert_close(y, ref, tol, tol, f"softmax causal={causal}")

    dy = torch.randn(R, C, device=DEV).to(dtype).contiguous()
    dx = OPS.softmax_bwd(y, dy, scale)
    yf = ref
    dot = (yf * dy.float()).sum(-1, keepdim=True)
    ref_dx = scale * yf * (dy.float() - dot)
    assert_close(dx, ref_dx, 0.03, 0.02, "softmax bwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rms_norm_kernel(dtype):
    torch.manual_seed(22)
    R, C = 128, 512
    x = torch.randn(R, C, device=DEV).to(dtype).contiguous()
    w = (torch.randn(C, device=DEV) * 0.3 + 1).to(dtype).contiguous()
    y, rstd = OPS.rms_fwd(x, w, 1e-5)
    xf = x.float()
    ref_rstd = (xf.pow(2).mean(1) + 1e-5).rsqrt()
    ref = xf * ref_rstd[:, None] * w.float()
    tol = 1e-4 if dtype == torch.float32 else 0.03
    assert_close(y, ref, tol, tol, "rms fwd")
    dy = torch.randn(R, C, device=DEV).to(dtype).contiguous()
    dx, dw = OPS.rms_bwd(x, dy, w, rstd)
    xr = xf.detach().requires_grad_(True)
    wr = w.float().detach().requires_grad_(True)
    rr = (xr.pow(2).mean(1, keepdim=True) + 1e-5).rsqrt()
    (xr * rr * wr).backward(dy.float())
    tol = 1e-3 if dtype == torch.float32 else 0.05
    assert_close(dx, xr.grad, tol, tol, "rms dx")
    assert_close(dw, wr.grad, tol, tol * R**0.5, "rms dw")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rope_kernel(dtype):
    from baton_amd.ops import functional as BF

    torch.manual_seed(23)
    B, S, H, D = 2, 32, 4, 64
    cos, sin = BF.rope_tables(S, D, device=DEV)
    x = torch.randn(B, S, H, D, device=DEV).to(dtype).contiguous()
    y = OPS.rope(x, cos, sin, False)
    # reference: CPU fallback path
    ref = BF.RoPEFn._cpu(x.cpu(), cos.cpu(), sin.cpu(), inverse=False)
    tol = 1e-5 if dtype == torch.float32 else 0.02
    assert_close(y.cpu(), ref, tol, tol, "rope fwd")
    # inverse undoes forward
    back = OPS.rope(y, cos, sin, True)
    assert_close(back, x.float(), 0.02, 0.02, "rope inverse")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_silu_mul_kernel(dtype):
    torch.manual_seed(24)
    a = torch.randn(5000, device=DEV).to(dtype).contiguous()
    b = torch.randn(5000, device=DEV).to(dtype).contiguous()
    y = OPS.silu_mul_fwd(a, b)
    ref = torch.nn.functional.silu(a.float()) * b.float()
    tol = 1e-5 if dtype == torch.float32 else 0.03
    assert_close(y, ref, tol, tol, "silu_mul")
    dy = torch.randn(5000, device=DEV).to(dtype).contiguous()
    da, db = OPS.silu_mul_bwd(dy, a, b)
    ar = a.float().detach().requires_grad_(True)
    br = b.float().detach().requires_grad_(True)
    (torch.nn.functional.silu(ar) * br).backward(dy.float())
    assert_close(da, ar.grad, 0.04, 0.03, "silu_mul da")
    assert_close(db, br.grad, 0.04, 0.03, "silu_mul db")


def test_bert_tiny_gpu_step():
    from baton_amd.models.bert import bert_tiny, make_synthetic_mlm
    from baton_amd.ops.optim import FusedAdam

    torch.manual_seed(25)
    m = bert_tiny().to(DEV).to(torch.bfloat16)
    # LN/Linear-bias params get re-pinned; embeddings stay bf16
    ids, labels = make_synthetic_mlm(8, 32, vocab_size=512)
    ids, labels = ids.to(DEV), labels.to(DEV)
    hist = m.train_round(ids, labels, n_epoch=3)
    assert all(v == v for v in hist), f"NaN: {hist}"
    assert hist[-1] < hist[0], f"MLM not learning on GPU: {hist}"


def test_llama_tiny_gpu_step():
    from baton_amd.models.llama import (
        LlamaForCausalLM, llama_tiny_config, make_synthetic_clm)

    torch.manual_seed(26)
    cfg = llama_tiny_config()
    m = LlamaForCausalLM(cfg).to(DEV).to(torch.bfloat16)
    m.rope_cos = m.rope_cos.float()
    m.rope_sin = m.rope_sin.float()
    ids, labels = make_synthetic_clm(4, 32, cfg.vocab_size)
    ids, labels = ids.to(DEV), labels.to(DEV)
    base_before = m.layers[0].attn.q_proj.weight.detach().clone()
    hist = m.train_round(ids, labels, n_epoch=3)
    assert all(v == v for v in hist), f"NaN: {hist}"
    assert hist[-1] < hist[0] + 1e-3, f"CLM not learning on GPU: {hist}"
    assert torch.equal(base_before, m.layers[0].attn.q_proj.weight.detach())


@pytest.mark.parametrize(
    "M,N,K,layout",
    [
        (2048, 16, 4096, 0),   # skinny-N NT (LoRA adapter fwd, 128x32 geom)
        (2048, 16, 4096, 1),   # skinny-N NN + split-K route
        (768, 768, 4096, 2),   # TN -> transpose + NT split-K route
        (512, 30522, 768, 0),  # unaligned-N vocab NT (edge tiles)
        (4096, 768, 30522, 1), # NN with unaligned K (vocab decoder dgrad)
    ],
)
def test_gemm_router_paths(M, N, K, layout):
    """Regression net over the GEMM dispatch routes (geometry selection,
    transpose routing, split-K): each exercised shape vs torch fp32."""
    torch.manual_seed(30 + layout)
    dt = torch.bfloat16
    if layout == 0:
        A = torch.randn(M, K, device=DEV).to(dt).contiguous()
        B = torch.randn(N, K, device=DEV).to(dt).contiguous()
        ref = A.float() @ B.float().t()
    elif layout == 1:
        A = torch.randn(M, K, device=DEV).to(dt).contiguous()
        B = torch.randn(K, N, device=DEV).to(dt).contiguous()
        ref = A.float() @ B.float()
    else:
        A = torch.randn(K, M, device=DEV).to(dt).contiguous()
        B = torch.randn(K, N, device=DEV).to(dt).contiguous()
        ref = A.float().t() @ B.float()
    want = {
        (2048, 16, 4096, 0): "TwoPhaseSplitK",
        (2048, 16, 4096, 1): "TwoPhaseSplitK",
        (768, 768, 4096, 2): "G9Slab",
        (512, 30522, 768, 0): "TwoPhase",
        (4096, 768, 30522, 1): "TwoPhaseSplitK",
    }[(M, N, K, layout)]
    assert OPS.gemm_plan(M, N, K, layout=layout)["kind"] == want
    C = OPS.gemm(A, B, layout)
    assert_close(C, ref, 0.05, 0.06 * K**0.5, f"router M{M} N{N} K{K} l{layout}")


def test_gemm_batched_gqa_group():
    """GQA b_group: 4 query heads share each KV batch; vs expanded bmm."""
    torch.manual_seed(40)
    nb, g, S, D = 8, 4, 64, 64
    q = torch.randn(nb, S, D, device=DEV, dtype=torch.bfloat16).contiguous()
    k = torch.randn(nb // g, S, D, device=DEV, dtype=torch.bfloat16).contiguous()
    C = OPS.gemm_batched(q, k, 0, False, 1.0, g)
    kx = k.float().repeat_interleave(g, dim=0)
    ref = torch.bmm(q.float(), kx.transpose(1, 2))
    assert_close(C, ref, 0.05, 0.05 * D**0.5, "gqa NT")
    p = torch.randn(nb, S, S, device=DEV, dtype=torch.bfloat16).contiguous()
    v = torch.randn(nb // g, S, D, device=DEV, dtype=torch.bfloat16).contiguous()
    O = OPS.gemm_batched(p, v, 1, False, 1.0, g)
    vx = v.float().repeat_interleave(g, dim=0)
    ref = torch.bmm(p.float(), vx)
    assert_close(O, ref, 0.05, 0.05 * S**0.5, "gqa NN")


def test_colsum_kernel():
    torch.manual_seed(41)
    x = torch.randn(4096, 768, device=DEV, dtype=torch.bfloat16).contiguous()
    out = OPS.colsum(x)
    ref = x.float().sum(0)
    assert_close(out, ref, 0.01, 0.01 * 4096**0.5, "colsum")


def test_gemm_nt_8phase_path():
    """Full-256-tile bf16 NT shapes vs torch fp32. The two small ones sit
    far below the 160-block gate of the deep-pipelined kernel and run the
    2-phase kernel; the long-K one takes the g9 split-K slab route."""
    for (M, N, K), kind in [((256, 256, 64), "TwoPhase"),
                            ((512, 768, 128), "TwoPhase"),
                            ((1024, 512, 4096), "G9Slab")]:
        assert OPS.gemm_plan(M, N, K)["kind"] == kind
        torch.manual_seed(50 + K)
        A = torch.randn(M, K, device=DEV, dtype=torch.bfloat16).contiguous()
        B = torch.randn(N, K, device=DEV, dtype=torch.bfloat16).contiguous()
        C = OPS.gemm(A, B, 0)
        ref = A.float() @ B.float().t()
        assert_close(C, ref, 0.05, 0.05 * K**0.5, f"8ph {M}x{N}x{K}")


def test_gemm_nt_8phase_large_grid():
    """Non-split 8-phase NT ABOVE the min-blocks routing gate (160 tiles:
    the shapes in test_gemm_nt_8phase_path fall back to the 2-phase
    kernel). Regression for the g9 quadrant-2 B-fragment-set bug, which
    only this route exercised."""
    torch.manual_seed(51)
    M, N = 4096, 2560                # (4096/256)*(2560/256) = 160 blocks
    for K in (512, 448):             # 448 = 7 K-tiles: odd B-parity tail
        assert OPS.gemm_plan(M, N, K)["kind"] == "G9"
        A = torch.randn(M, K, device=DEV, dtype=torch.bfloat16).contiguous()
        B = torch.randn(N, K, device=DEV, dtype=torch.bfloat16).contiguous()
        C = OPS.gemm(A, B, 0)
        ref = A.float() @ B.float().t()
        assert_close(C, ref, 0.05, 0.05 * K**0.5, f"8ph large grid K{K}")


def test_batchnorm_eval_path_gpu():
    """Eval-mode BN normalizes with running stats (bn_fwd_eval kernel)."""
    from baton_amd.ops.modules import BatonBatchNorm2d

    torch.manual_seed(60)
    bn = BatonBatchNorm2d(32).to(DEV)
    ref = torch.nn.BatchNorm2d(32).to(DEV)
    x = torch.randn(4, 8, 8, 32, device=DEV)
    bn.train(); ref.train()
    bn(x)
    ref(x.permute(0, 3, 1, 2))
    bn.eval(); ref.eval()
    y = bn(x)
    yr = ref(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert_close(y, yr, 1e-4, 1e-4, "bn eval")


def test_resnet_eval_mode_gpu():
    from baton_amd.models.resnet import make_synthetic_cifar, resnet18

    torch.manual_seed(61)
    m = resnet18().to(DEV).to(torch.bfloat16)
    x, y = make_synthetic_cifar(8, dtype=torch.bfloat16)
    m.train(); m(x.to(DEV))          # populate running stats
    m.eval()
    with torch.no_grad():
        logits = m(x.to(DEV))
    assert torch.isfinite(logits.float()).all()


def test_gemm_nt_8phase_ragged_m():
    """Ragged token count (M % 256 != 0) with a small tile grid and long
    K: 16 x 4 tiles < 256, so this is the 2-phase atomic split-K (ragged M
    rules out the slab route). The G9 main block + remainder split is
    covered by test_gemm_nt_uncovered_routes."""
    torch.manual_seed(70)
    M, N, K = 2048 - 48, 512, 1024   # M = 2000: 7 full 256-tiles + 208 rows
    assert OPS.gemm_plan(M, N, K)["kind"] == "TwoPhaseSplitK"
    A = torch.randn(M, K, device=DEV, dtype=torch.bfloat16).contiguous()
    B = torch.randn(N, K, device=DEV, dtype=torch.bfloat16).contiguous()
    C = OPS.gemm(A, B, 0)
    ref = A.float() @ B.float().t()
    assert_close(C, ref, 0.05, 0.05 * K**0.5, "8ph ragged M")


@pytest.mark.parametrize(
    "M,N,K,kind",
    [
        (256, 256, 1152, "G8Slab"),   # k_chunk 288 = 9 k-halves: not g9's
        (256, 256, 1280, "G9Slab"),   # k_chunk 320 = 5 K-tiles: odd tail
        (2608, 4096, 192, "G9"),      # 2560 rows G9 + 48 rows 2-phase
    ],
)
def test_gemm_nt_uncovered_routes(M, N, K, kind):
    """The smallest shapes that reach the g8 slab kernel, the g9 slab
    odd-K-tile tail, and the ragged-M G9 main block + 2-phase remainder."""
    plan = OPS.gemm_plan(M, N, K)
    assert plan["kind"] == kind
    if M % 256:
        assert plan["m_main"] == M // 256 * 256
        assert plan["remainder"]["kind"] == "TwoPhase"
    torch.manual_seed(72)
    A = torch.randn(M, K, device=DEV, dtype=torch.bfloat16).contiguous()
    B = torch.randn(N, K, device=DEV, dtype=torch.bfloat16).contiguous()
    C = OPS.gemm(A, B, 0)
    ref = A.float() @ B.float().t()
    assert_close(C, ref, 0.05, 0.05 * K**0.5, f"{kind} {M}x{N}x{K}")


def test_linear_frozen_weight_t_path():
    """LinearFn with a cached W^T (frozen weights) must match the NN dgrad."""
    from baton_amd.ops import functional as BF

    torch.manual_seed(71)
    x = torch.randn(512, 256, device=DEV, dtype=torch.bfloat16,
                    requires_grad=True)
    w = torch.randn(384, 256, device=DEV, dtype=torch.bfloat16)
    wt = w.t().contiguous()
    y = BF.linear(x, w, weight_t=wt)
    dy = torch.randn_like(y)
    y.backward(dy)
    gx_cached = x.grad.clone()
    x.grad = None
    y2 = BF.linear(x, w)
    y2.backward(dy)
    assert_close(gx_cached, x.grad, 0.03, 0.3, "weight_t dgrad")
    assert_close(y, y2, 1e-6, 1e-6, "weight_t fwd identical")


# ---- flash attention (flash.hip) -------------------------------------------

def _ref_attn(q, k, v, causal):
    """fp32 torch reference on [B,S,h,dh] layouts."""
    qr = q.float().permute(0, 2, 1, 3)
    kr = k.float().permute(0, 2, 1, 3)
    vr = v.float().permute(0, 2, 1, 3)
    o = torch.nn.functional.scaled_dot_product_attention(qr, kr, vr,
                                                         is_causal=causal)
    return o.permute(0, 2, 1, 3)


@pytest.mark.parametrize(
    "B,S,h,kvh,dh,causal",
    [
        (4, 128, 12, 12, 64, False),    # BERT-base shape
        (2, 512, 8, 2, 128, True),      # Llama-like GQA causal
        (2, 96, 4, 4, 32, False),       # S not a multiple of 64 (tail tile)
        (1, 200, 4, 2, 64, True),       # odd S + causal + GQA
        (2, 64, 4, 4, 32, True),        # single q-block causal
    ],
)
def test_flash_attention_vs_torch(B, S, h, kvh, dh, causal):
    import baton_amd.ops.functional as BF

    torch.manual_seed(7)
    q = (torch.randn(B, S, h, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
    k = (torch.randn(B, S, kvh, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
    v = (torch.randn(B, S, kvh, dh, device=DEV).bfloat16() * 0.5).requires_grad_(True)
    o = BF.attention_bshd(q, k, v, causal=causal)
    g = h // kvh
    qr = q.detach().float().requires_grad_(True)
    kr = k.detach().float().requires_grad_(True)
    vr = v.detach().float().requires_grad_(True)
    kx = kr.repeat_interleave(g, dim=2) if g > 1 else kr
    vx = vr.repeat_interleave(g, dim=2) if g > 1 else vr
    ref_o = _ref_attn(qr, kx, vx, causal)
    assert_close(o, ref_o, 0.03, 0.03, "flash fwd")
    do = torch.randn_like(ref_o)
    ref_o.backward(do)
    o.backward(do.to(o.dtype))
    assert_close(q.grad, qr.grad, 0.05, 0.05, "flash dq")
    assert_close(k.grad, kr.grad, 0.05, 0.05, "flash dk")
    assert_close(v.grad, vr.grad, 0.05, 0.05, "flash dv")


def test_flash_matches_unfused_path():
    """Flash and the materialized-scores path agree on the same inputs
    (BATON_NO_FLASH toggles the legacy path)."""
    import os

    import baton_amd.ops.functional as BF

    torch.manual_seed(11)
    qkv = (torch.randn(2, 128, 3, 4, 64, device=DEV).bfloat16() * 0.5
           ).requires_grad_(True)
    o_flash = BF.attention_qkv(qkv, causal=False)
    o_flash.backward(torch.ones_like(o_flash))
    g_flash = qkv.grad.clone()
    qkv.grad = None
    os.environ["BATON_NO_FLASH"] = "1"
    try:
        o_leg = BF.attention_qkv(qkv, causal=False)
        o_leg.backward(torch.ones_like(o_leg))
    finally:
        os.environ.pop("BATON_NO_FLASH", None)
    assert_close(o_flash, o_leg, 0.03, 0.03, "flash vs legacy fwd")
    assert_close(g_flash, qkv.grad, 0.05, 0.08, "flash vs legacy bwd")


def test_flash_spiked_max_numerics():
    """Rule-26-style rescale test: one K row spiked against one Q row so
    the running max jumps mid-sequence; compare against an fp64 reference."""
    import baton_amd.ops.functional as BF

    torch.manual_seed(3)
    B, S, h, dh = 1, 256, 2, 64
    q = torch.randn(B, S, h, dh, device=DEV) * 0.5
    k = torch.randn(B, S, h, dh, device=DEV) * 0.5
    v = torch.randn(B, S, h, dh, device=DEV) * 0.5
    # spike: K row 200 aligned with Q row 10 -> its score dominates late
    k[0, 200, :, :] = q[0, 10, :, :] * 4.0
    qb, kb, vb = q.bfloat16(), k.bfloat16(), v.bfloat16()
    o = BF.attention_bshd(qb, kb, vb, causal=False)
    qd = qb.double().permute(0, 2, 1, 3)
    kd = kb.double().permute(0, 2, 1, 3)
    vd = vb.double().permute(0, 2, 1, 3)
    s = (qd @ kd.transpose(-1, -2)) / (dh ** 0.5)
    ref = (torch.softmax(s, dim=-1) @ vd).permute(0, 2, 1, 3)
    assert_close(o, ref, 0.03, 0.03, "flash spiked max")


# ---- fused residual-add norms ----------------------------------------------

def test_layer_norm_add_vs_compose():
    import baton_amd.ops.functional as BF

    torch.manual_seed(5)
    x = (torch.randn(64, 768, device=DEV).bfloat16()).requires_grad_(True)
    r = (torch.randn(64, 768, device=DEV).bfloat16()).requires_grad_(True)
    w = torch.randn(768, device=DEV).bfloat16().requires_grad_(True)
    b = torch.randn(768, device=DEV).bfloat16().requires_grad_(True)
    y = BF.layer_norm_add(x, r, w, b, 1e-12)
    x2 = x.detach().clone().requires_grad_(True)
    r2 = r.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    b2 = b.detach().clone().requires_grad_(True)
    y2 = BF.layer_norm(x2 + r2, w2, b2, 1e-12)
    assert_close(y, y2, 0.02, 0.02, "ln_add fwd")
    g = torch.randn_like(y)
    y.backward(g)
    y2.backward(g)
    assert_close(x.grad, x2.grad, 0.03, 0.03, "ln_add dx")
    assert_close(r.grad, r2.grad, 0.03, 0.03, "ln_add dres")
    assert_close(w.grad, w2.grad, 0.03, 0.05, "ln_add dw")
    assert_close(b.grad, b2.grad, 0.03, 0.05, "ln_add db")


def test_add_rms_norm_vs_compose():
    import baton_amd.ops.functional as BF

    torch.manual_seed(6)
    x = (torch.randn(64, 512, device=DEV).bfloat16()).requires_grad_(True)
    r = (torch.randn(64, 512, device=DEV).bfloat16()).requires_grad_(True)
    w = torch.randn(512, device=DEV).bfloat16().requires_grad_(True)
    y, z = BF.add_rms_norm(x, r, w, 1e-6)
    x2 = x.detach().clone().requires_grad_(True)
    r2 = r.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    z2 = x2 + r2
    y2 = BF.rms_norm(z2, w2, 1e-6)
    assert_close(y, y2, 0.02, 0.02, "add_rms fwd y")
    assert_close(z, z2, 0.02, 0.02, "add_rms fwd z")
    g1 = torch.randn_like(y)
    g2 = torch.randn_like(z)
    # grads flow through BOTH outputs (z is the residual stream)
    torch.autograd.backward([y, z], [g1, g2])
    torch.autograd.backward([y2, z2], [g1, g2])
    assert_close(x.grad, x2.grad, 0.03, 0.03, "add_rms dx")
    assert_close(r.grad, r2.grad, 0.03, 0.03, "add_rms dres")
    assert_close(w.grad, w2.grad, 0.03, 0.05, "add_rms dw")


def test_fused_zero_grad_sgd_trajectory():
    """Arena + fused-zero optimizer matches an explicit zero_grad loop."""
    from baton_amd.ops.optim import FusedSGD
    from baton_amd.runtime.arena import FlatParamArena

    def run(fused):
        torch.manual_seed(9)
        m = torch.nn.Sequential(
            torch.nn.Linear(32, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8)
        ).to(DEV).bfloat16()
        arena = FlatParamArena(m)
        opt = FusedSGD.from_arena(arena, lr=0.05, momentum=0.9)
        if not fused:
            opt._fused_zero = False
        x = torch.randn(16, 32, device=DEV).bfloat16()
        t = torch.randn(16, 8, device=DEV).bfloat16()
        for _ in range(5):
            opt.zero_grad()
            loss = (m(x).float() - t.float()).square().mean()
            loss.backward()
            opt.step()
        return [p.detach().float().clone() for p in m.parameters()]

    a = run(True)
    b = run(False)
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb), "fused-zero trajectory diverged"


# ---- 8-phase split-K slab wgrad path ---------------------------------------

@pytest.mark.parametrize("M,N,K", [(768, 768, 16384), (3072, 768, 8192),
                                   (2304, 768, 16384)])
def test_gemm_tn_splitk_slab_vs_torch(M, N, K):
    """BERT wgrad shapes: TN long-K skinny tiles route to the 8-phase
    split-K slab kernel (per-slice fp32 partials + reduce, no atomics)."""
    torch.manual_seed(17)
    A = (torch.randn(K, M, device=DEV) * 0.3).bfloat16()   # dy [K=BS, M=outf]
    B = (torch.randn(K, N, device=DEV) * 0.3).bfloat16()   # x  [K=BS, N=inf]
    assert OPS.gemm_plan(M, N, K, layout=2)["kind"] == "G9Slab"
    C = OPS.gemm(A, B, 2)                                   # TN: A^T @ B
    ref = A.float().t() @ B.float()
    assert_close(C, ref, 0.02, 0.5, f"tn splitk {M}x{N}x{K}")


# ---- 8-phase conv (conv8.hip) ----------------------------------------------

@pytest.mark.parametrize(
    "N,H,W,Cin,Cout,K,s,p",
    [
        (256, 16, 16, 256, 256, 3, 1, 1),   # fwd+dgrad 8ph eligible
        (512, 8, 8, 256, 512, 3, 1, 1),     # layer4-like
        (256, 16, 16, 128, 256, 1, 2, 0),   # 1x1 stride-2 downsample (fwd)
    ],
)
def test_conv_8ph_vs_torch(N, H, W, Cin, Cout, K, s, p):
    torch.manual_seed(21)
    x = (torch.randn(N, H, W, Cin, device=DEV) * 0.5).bfloat16()
    w = (torch.randn(Cout, K, K, Cin, device=DEV) * 0.1).bfloat16()
    y = OPS.conv_fwd(x, w, s, p)
    xn = x.float().permute(0, 3, 1, 2)
    wn = w.float().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xn, wn, stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    assert_close(y, ref, 0.05, 0.06 * (Cin * K * K) ** 0.5, "conv8 fwd")

    HO, WO = ref.shape[1], ref.shape[2]
    dy = (torch.randn(N, HO, WO, Cout, device=DEV) * 0.1).bfloat16()
    dx = OPS.conv_dgrad(dy, w, H, W, s, p)
    dyn = dy.float().permute(0, 3, 1, 2)
    refdx = torch.nn.grad.conv2d_input((N, Cin, H, W), wn, dyn, stride=s,
                                       padding=p)
    refdx = refdx.permute(0, 2, 3, 1).contiguous()
    assert_close(dx, refdx, 0.05, 0.06 * (Cout * K * K) ** 0.5, "conv8 dgrad")


def test_conv_wgrad_1x1_slab_splitk_vs_torch():
    """256-divisible 1x1 stride-1 wgrad routes through transpose-x +
    8-phase split-K slab kernel."""
    torch.manual_seed(23)
    N, H, W, Cin, Cout = 64, 16, 16, 256, 512
    x = (torch.randn(N, H, W, Cin, device=DEV) * 0.5).bfloat16()
    dy = (torch.randn(N, H, W, Cout, device=DEV) * 0.1).bfloat16()
    npix = N * H * W
    # the wgrad is the NT problem dy_t[Cout, P] @ x_t[Cin, P]^T
    assert OPS.gemm_plan(Cout, Cin, npix)["kind"] == "G9Slab"
    dw = OPS.conv_wgrad(dy, x, 1, 1, 1, 0, True)
    xn = x.float().permute(0, 3, 1, 2)
    dyn = dy.float().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, 1, 1), dyn, stride=1,
                                      padding=0)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    assert_close(dw, ref, 0.05, 0.06 * npix**0.5, "1x1 slab wgrad")


def test_bn_add_relu_fused_vs_compose():
    """relu(bn(x) + res) fused into the BN normalize pass, fwd + bwd.

    Gradients are checked against a torch fp32 reference built from the
    FUSED forward's own ReLU mask: the fused path rounds bn(x)+res to
    bf16 once where a composed bn -> add_relu rounds twice, so elements
    within rounding of zero can legitimately sit on opposite sides of the
    mask between the two implementations."""
    import baton_amd.ops.functional as BF

    torch.manual_seed(31)
    M, C = 512, 128
    x = (torch.randn(M, C, device=DEV) * 0.7).bfloat16().requires_grad_(True)
    r = (torch.randn(M, C, device=DEV) * 0.7).bfloat16().requires_grad_(True)
    g = torch.rand(C, device=DEV) + 0.5
    b = torch.randn(C, device=DEV) * 0.1
    g1 = g.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    y = BF.BatchNormAddReLUFn.apply(x, r, g1, b1, rm, rv, 0.1, 1e-5)

    # forward vs composed (mask-free comparison of values)
    xf = x.detach().float()
    mean = xf.mean(0)
    var = xf.var(0, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    xhat = (xf - mean) * rstd
    y_ref = (xhat * g + b + r.detach().float()).clamp_min(0)
    assert_close(y, y_ref, 0.03, 0.03, "bn_add_relu fwd")
    assert_close(rm, mean * 0.1, 1e-3, 1e-3, "running mean")

    dy = torch.randn_like(y)
    y.backward(dy)
    # reference gradients from the fused forward's OWN mask
    mask = (y.detach().float() > 0).float()
    md = dy.float() * mask
    sum_dy = md.sum(0)
    sum_dyx = (md * xhat).sum(0)
    dx_ref = rstd * g * (md - sum_dy / M - xhat * sum_dyx / M)
    assert_close(x.grad, dx_ref, 0.05, 0.05, "bn_add_relu dx")
    assert_close(r.grad, md, 0.02, 0.02, "bn_add_relu dres")
    assert_close(g1.grad, sum_dyx, 0.05, 0.2, "bn_add_relu dgamma")
    assert_close(b1.grad, sum_dy, 0.05, 0.2, "bn_add_relu dbeta")


@pytest.mark.parametrize(
    "N,H,W,Cin,Cout",
    [
        (16, 32, 32, 64, 64),     # layer1-like (halo fwd + dgrad)
        (16, 16, 16, 128, 128),   # layer2-like
        (4, 32, 32, 96, 64),      # Cin%32 only (fwd); dgrad falls back
        (2, 16, 16, 64, 192),     # Cout not 64-mult for dgrad N tile -> ok fwd
    ],
)
def test_conv_halo_vs_torch(N, H, W, Cin, Cout):
    """Shared-halo 3x3 stride-1 conv path (small-channel layers)."""
    torch.manual_seed(41)
    x = (torch.randn(N, H, W, Cin, device=DEV) * 0.5).bfloat16()
    w = (torch.randn(Cout, 3, 3, Cin, device=DEV) * 0.1).bfloat16()
    y = OPS.conv_fwd(x, w, 1, 1)
    xn = x.float().permute(0, 3, 1, 2)
    wn = w.float().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xn, wn, stride=1, padding=1)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    assert_close(y, ref, 0.05, 0.06 * (Cin * 9) ** 0.5, "halo fwd")

    dy = (torch.randn(N, H, W, Cout, device=DEV) * 0.1).bfloat16()
    dx = OPS.conv_dgrad(dy, w, H, W, 1, 1)
    dyn = dy.float().permute(0, 3, 1, 2)
    refdx = torch.nn.grad.conv2d_input((N, Cin, H, W), wn, dyn, stride=1,
                                       padding=1)
    refdx = refdx.permute(0, 2, 3, 1).contiguous()
    assert_close(dx, refdx, 0.05, 0.06 * (Cout * 9) ** 0.5, "halo dgrad")

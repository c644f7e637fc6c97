"""Every GEMM route and epilogue through ``gemm`` / ``gemm_batched`` against
a float64 reference on the CPU, with an elementwise bound that has no free
constants (the form tests/test_conv_dgrad_strided.py uses).

With fp32 ``bias`` and ``C0`` the contents of ``C_in`` before the call,

    ref   = alpha op(A) op(B) + beta C0 + bias        (float64; relu after)
    mag   = |alpha| |op(A)| |op(B)| + |beta| |C0| + |bias|
    |got - ref| <= (K + 3) 2^-23 mag + store |ref|

(K + 3) 2^-23 is the (n-1) u sum|t_i| summation bound with u = 2^-24,
doubled for MFMA-internal rounding and the rounded products of the fp32
kernel; the +3 is the alpha multiply, the beta fma and the bias add. It
holds for any summation order, so the atomic and slab split-K routes need
nothing extra. ``store`` is 2^-8, the unit roundoff of one round-to-nearest
bf16 store, and 0 for an fp32 result. alpha and beta are exact in fp32.
An honest fp32 implementation sits at 0.7 - 1.0 of this bound for bf16
results (the store term dominates) and below 0.05 for fp32 results; a
truncating store reaches 1.5 - 2, a bias rounded to bf16, a shifted bias or
a dropped k element 4 - 10^4.

Every case first asserts the plan (tests/test_gemm_plan.py derives the
routing rules), so a planner change cannot quietly turn a case into a test
of another kernel. What the cases are for:

* 2-phase dense epilogue (gemm.hip) on the 128x64, 64x128, 128x32 and
  128x128 tiles, ragged in M and N. K = 104 and 40 stage full k-steps with
  global_load_lds and the K tail through registers in the same block;
  K = 100 has no 16-byte rows and stages through registers only.
* G9 (gemm8.hip): K = 64 and 128 are the one- and two-tile prologue
  branches, M = 4136 puts 40 remainder rows on the 2-phase kernel with the
  same bias.
* split routes: 1040 = 32 slices of 32 and one of 16; the slab routes with
  bf16 and fp32 results and behind the TN / NN re-layouts.
* the combinations without a kernel are refused before any launch."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"

NT, NN, TN = 0, 1, 2
BF16, FP32 = torch.bfloat16, torch.float32


def case(M, N, K, layout=NT, dtype=BF16, bias=False, relu=False, alpha=1.0,
         beta=0.0, c_in=None, out_f32=False, direct=False, **plan):
    """c_in: None, "rand" (C0 = random values) or "nan" (beta must be 0: the
    kernel may not read C). ``plan`` holds the expected gemm_plan entries."""
    return dict(M=M, N=N, K=K, layout=layout, dtype=dtype, bias=bias,
                relu=relu, alpha=alpha, beta=beta, c_in=c_in, out_f32=out_f32,
                direct=direct, plan=plan)


def dense(tile, **kw):
    return dict(kind="TwoPhase", tile=tile, splits=1, transpose_a=False,
                transpose_b=False, **kw)


T_128x64 = dense((128, 64), grid=(3, 2, 1))      # 200 x 136
T_64x128 = dense((64, 128), grid=(2, 2, 1))      # 72 x 200
T_128x32 = dense((128, 32), grid=(1, 2, 1))      # 200 x 24
T_128x128 = dense((128, 128), grid=(24, 17, 1))  # 2056 x 3000: 408 tiles
G9 = dict(kind="G9", tile=(256, 256), grid=(10, 16, 1), m_main=4096,
          transpose_a=False, transpose_b=False)
# 136 x 72 x 1040: 2 x 2 tiles of 128 x 64, 33 slices, the last 16 wide
SPLITK = dict(kind="TwoPhaseSplitK", tile=(128, 64), grid=(2, 2, 33),
              splits=33, k_chunk=32)
SLAB = dict(kind="G9Slab", layout_=NT, splits=4, k_chunk=256)

CASES = {}
for dt, tag in ((BF16, "bf16"), (FP32, "fp32")):
    CASES.update({
        f"t128x64_bias_{tag}": case(200, 136, 104, dtype=dt, bias=True,
                                    **T_128x64),
        f"t128x64_alpha_bias_{tag}": case(200, 136, 104, dtype=dt, bias=True,
                                          alpha=0.5, **T_128x64),
        f"t128x64_alpha_beta_{tag}": case(200, 136, 104, dtype=dt, alpha=2.0,
                                          beta=1.0, c_in="rand", **T_128x64),
        f"t128x64_bias_relu_{tag}": case(200, 136, 104, dtype=dt, bias=True,
                                         relu=True, **T_128x64),
        f"t128x64_alpha_beta_bias_{tag}": case(
            200, 136, 104, dtype=dt, alpha=-1.5, beta=0.5, c_in="rand",
            bias=True, **T_128x64),
        # beta = 0: C is written, never read
        f"t128x64_nan_c_in_{tag}": case(200, 136, 104, dtype=dt, c_in="nan",
                                        **T_128x64),
        f"t64x128_bias_relu_{tag}": case(72, 200, 100, dtype=dt, bias=True,
                                         relu=True, **T_64x128),
        f"t64x128_beta_{tag}": case(72, 200, 100, dtype=dt, beta=1.0,
                                    c_in="rand", **T_64x128),
        f"t128x32_bias_{tag}": case(200, 24, 40, dtype=dt, bias=True,
                                    **T_128x32),
        f"t128x32_alpha_{tag}": case(200, 24, 40, dtype=dt, alpha=0.5,
                                     **T_128x32),
    })
CASES.update({
    "t128x128_alpha_beta_bias": case(2056, 3000, 40, alpha=2.0, beta=1.0,
                                     c_in="rand", bias=True, **T_128x128),
    # B is 28 KiB: NN stays native; plain TN is re-laid-out to NT unless the
    # caller forbids it or wants fp32 out
    "nn_plain": case(200, 136, 104, NN, layout_=NN, **T_128x64),
    "tn_relayout": case(200, 136, 104, TN, kind="TwoPhase", tile=(128, 64),
                        layout_=NT, transpose_a=True, transpose_b=True),
    "tn_native_direct": case(200, 136, 104, TN, direct=True, layout_=TN,
                             **T_128x64),
    "tn_native_out_f32": case(200, 136, 104, TN, out_f32=True, layout_=TN,
                              **T_128x64),
    "k1_bias": case(200, 136, 1, bias=True, **T_128x64),
    "k8_bias": case(200, 136, 8, bias=True, **T_128x64),
    # G9: 16 x 10 = 160 blocks, exactly the gate
    "g9_1tile_bias": case(4096, 2560, 64, bias=True, remainder=None, **G9),
    "g9_1tile_nan_c_in": case(4096, 2560, 64, c_in="nan", remainder=None,
                              **G9),
    "g9_shape_relu_is_2ph": case(4096, 2560, 64, relu=True,
                                 **dense((128, 128), grid=(20, 32, 1))),
    "g9_2tile_alpha": case(4096, 2560, 128, alpha=0.5, remainder=None, **G9),
    "g9_ragged_m_alpha_bias": case(
        4136, 2560, 192, bias=True, alpha=-1.5,
        remainder=dict(kind="TwoPhase", tile=(64, 128), grid=(20, 1, 1),
                       m_main=40), **G9),
    "splitk_nt": case(136, 72, 1040, layout_=NT, **SPLITK),
    "splitk_nt_fp32": case(136, 72, 1040, dtype=FP32, layout_=NT, **SPLITK),
    "splitk_nn": case(136, 72, 1040, NN, layout_=NN, transpose_b=False,
                      **SPLITK),
    "splitk_tn_native_out_f32": case(136, 72, 1040, TN, out_f32=True,
                                     layout_=TN, transpose_a=False, **SPLITK),
    "splitk_tn_relayout": case(136, 72, 1040, TN, layout_=NT,
                               transpose_a=True, transpose_b=True, **SPLITK),
    "splitk_nt_out_f32": case(136, 72, 1040, out_f32=True, layout_=NT,
                              **SPLITK),
    # alpha != 1 is not plain: dense, a 1040-long K loop with a 16-wide tail
    "long_k_alpha_is_dense": case(136, 72, 1040, alpha=0.5,
                                  **dense((128, 64), grid=(2, 2, 1))),
    "slab_nt": case(256, 256, 1024, grid=(1, 1, 4), **SLAB),
    "slab_nt_out_f32": case(256, 256, 1024, out_f32=True, grid=(1, 1, 4),
                            **SLAB),
    "slab_tn_relayout": case(256, 256, 1024, TN, grid=(1, 1, 4),
                             transpose_a=True, transpose_b=True, **SLAB),
    # B is exactly 1 MiB: the NN re-layout threshold
    "slab_nn_relayout": case(256, 512, 1024, NN, grid=(2, 1, 4),
                             transpose_a=False, transpose_b=True, **SLAB),
})


@functools.lru_cache(maxsize=3)
def operands(M, N, K, layout, dtype):
    """Inputs rounded to the compute dtype, op(A) op(B) and |op(A)| |op(B)|
    in float64, an fp32 bias and raw C0 values; shared by the epilogue
    variants of a shape (adjacent in CASES) and never modified."""
    g = torch.Generator().manual_seed(977 * M + 31 * N + K + 7 * layout)
    A = torch.randn((K, M) if layout == TN else (M, K), generator=g).to(dtype)
    B = torch.randn((N, K) if layout == NT else (K, N), generator=g).to(dtype)
    bias = torch.randn(N, generator=g).mul(4.0)
    C0 = torch.randn(M, N, generator=g).mul(4.0)
    Ad = A.double().t() if layout == TN else A.double()
    Bd = B.double().t() if layout == NT else B.double()
    return A, B, bias, C0, Ad @ Bd, Ad.abs() @ Bd.abs()


def reference(c):
    """(A, B, bias, C0 in the output dtype, ref, bound) for a case."""
    A, B, bias, C0, P, Pabs = operands(c["M"], c["N"], c["K"], c["layout"],
                                       c["dtype"])
    out_dtype = FP32 if c["out_f32"] else c["dtype"]
    ref = c["alpha"] * P
    mag = abs(c["alpha"]) * Pabs
    if c["c_in"] == "rand":
        C0 = C0.to(out_dtype)
        ref = ref + c["beta"] * C0.double()
        mag = mag + abs(c["beta"]) * C0.double().abs()
    elif c["c_in"] == "nan":
        assert c["beta"] == 0.0
        C0 = torch.full((c["M"], c["N"]), float("nan"), dtype=out_dtype)
    else:
        C0 = None
    if c["bias"]:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    else:
        bias = None
    if c["relu"]:
        ref = ref.clamp_min(0.0)
    return A, B, bias, C0, ref, (c["K"] + 3) * 2.0 ** -23 * mag, out_dtype


def check_plan(got, want):
    want = dict(want)
    if "layout_" in want:
        want["layout"] = want.pop("layout_")
    for key, val in want.items():
        if key == "remainder" and val is not None:
            check_plan(got[key], val)
        else:
            assert got[key] == val, f"plan {key}: {got[key]!r} != {val!r}: {got}"


def check(tag, got, ref, bound, out_dtype):
    assert torch.isfinite(got).all(), f"{tag}: non-finite result"
    store = 0.0 if out_dtype == FP32 else 2.0 ** -8
    err = (got.double() - ref).abs()
    lim = bound + store * ref.abs()
    ratio = torch.where(lim > 0, err / lim, (err > 0).double() * 2).max().item()
    print(f"gemm_exact {tag}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{tag}: error is {ratio:.3f} x the bound"


@pytest.mark.parametrize("name", list(CASES))
def test_gemm(name):
    c = CASES[name]
    check_plan(OPS.gemm_plan(c["M"], c["N"], c["K"], layout=c["layout"],
                             bf16=c["dtype"] == BF16, out_f32=c["out_f32"],
                             has_bias=c["bias"], relu=c["relu"],
                             alpha=c["alpha"], beta=c["beta"],
                             direct=c["direct"]), c["plan"])
    A, B, bias, C0, ref, bound, out_dtype = reference(c)
    C_in = None if C0 is None else C0.to(DEV)
    got = OPS.gemm(A.to(DEV), B.to(DEV), c["layout"],
                   None if bias is None else bias.to(DEV), c["relu"],
                   c["out_f32"], c["alpha"], c["beta"], C_in, c["direct"])
    assert got.dtype == out_dtype and tuple(got.shape) == (c["M"], c["N"])
    if C_in is not None:
        # the result is C_in itself, written in place
        assert got.data_ptr() == C_in.data_ptr()
    check(name, got.cpu(), ref, bound, out_dtype)


# ---- gemm_batched ------------------------------------------------------------
# nb = 6 of 128 x 64 x 104: six tiles of 128 x 64, glds steps plus a register
# tail on every layout that can use glds.

NB, BM, BN, BK = 6, 128, 64, 104
BATCHED = {
    "nt_alpha": (NT, False, 1),
    "nn_alpha": (NN, False, 1),
    "tn_alpha": (TN, False, 1),
    "tn_alpha_out_f32": (TN, True, 1),
    # six A batches over two B batches
    "nt_alpha_b_group3": (NT, False, 3),
}


@pytest.mark.parametrize("name", list(BATCHED))
def test_gemm_batched(name):
    layout, out_f32, b_group = BATCHED[name]
    alpha = 0.5
    check_plan(OPS.gemm_plan(BM, BN, BK, layout=layout, out_f32=out_f32,
                             alpha=alpha, nbatch=NB, batched=True, direct=True),
               dense((128, 64), grid=(1, 1, NB), layout=layout))
    g = torch.Generator().manual_seed(5150 + 10 * layout + b_group)
    A = torch.randn((NB, BK, BM) if layout == TN else (NB, BM, BK),
                    generator=g).to(BF16)
    B = torch.randn((NB // b_group,) + ((BN, BK) if layout == NT else (BK, BN)),
                    generator=g).to(BF16)
    Ad = A.double().transpose(1, 2) if layout == TN else A.double()
    Bd = B.double().transpose(1, 2) if layout == NT else B.double()
    Bd = Bd.repeat_interleave(b_group, dim=0)
    ref = alpha * torch.bmm(Ad, Bd)
    bound = (BK + 3) * 2.0 ** -23 * alpha * torch.bmm(Ad.abs(), Bd.abs())
    got = OPS.gemm_batched(A.to(DEV), B.to(DEV), layout, out_f32, alpha,
                           b_group)
    out_dtype = FP32 if out_f32 else BF16
    assert got.dtype == out_dtype and tuple(got.shape) == (NB, BM, BN)
    check(f"batched {name}", got.cpu(), ref, bound, out_dtype)


# ---- refused combinations ----------------------------------------------------
# All of these raise before anything is allocated or launched.

def _ab(layout, M=200, N=136, K=104, dtype=BF16):
    A = torch.zeros((K, M) if layout == TN else (M, K), dtype=dtype, device=DEV)
    B = torch.zeros((N, K) if layout == NT else (K, N), dtype=dtype, device=DEV)
    return A, B


@pytest.mark.parametrize("layout", [NT, NN])
def test_gemm_refuses_dense_out_f32(layout):
    A, B = _ab(layout)
    with pytest.raises(RuntimeError, match="unsupported"):
        OPS.gemm(A, B, layout, out_f32=True)


@pytest.mark.parametrize("layout", [NN, TN])
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_gemm_refuses_relu_off_nt(layout, dtype):
    A, B = _ab(layout, dtype=dtype)
    with pytest.raises(RuntimeError, match="unsupported"):
        OPS.gemm(A, B, layout, relu=True)


@pytest.mark.parametrize("layout", [NT, NN])
def test_gemm_batched_refuses_out_f32(layout):
    A = torch.zeros(NB, BM, BK, dtype=BF16, device=DEV)
    B = torch.zeros((NB, BN, BK) if layout == NT else (NB, BK, BN), dtype=BF16,
                    device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        OPS.gemm_batched(A, B, layout, True)


def test_gemm_fp32_out_f32_is_a_noop():
    A, B = _ab(NT, dtype=FP32)
    assert OPS.gemm(A, B, NT, out_f32=True).dtype == FP32


def test_gemm_refuses_bad_c_in():
    A, B = _ab(NT)
    ok = torch.zeros(200, 136, dtype=BF16, device=DEV)
    bad = {
        "dtype": torch.zeros(200, 136, dtype=FP32, device=DEV),
        "device": torch.zeros(200, 136, dtype=BF16),
        "shape": torch.zeros(136, 200, dtype=BF16, device=DEV),
        "rank": torch.zeros(1, 200, 136, dtype=BF16, device=DEV),
        "strides": torch.zeros(200, 272, dtype=BF16, device=DEV)[:, ::2],
    }
    for what, C_in in bad.items():
        with pytest.raises(RuntimeError, match="C_in"):
            OPS.gemm(A, B, NT, beta=1.0, C_in=C_in)
        print(f"gemm_exact refused C_in with wrong {what}")
    assert OPS.gemm(A, B, NT, beta=1.0, C_in=ok).data_ptr() == ok.data_ptr()

"""``softmax_fwd`` / ``softmax_bwd`` (attention.hip) on every route, bf16 and
fp32, against float64 built from the stored inputs, with an elementwise bound
(the form of tests/test_gemm_exact.py).

With z = scale x (exact here: scale = 2^-3), the causal mask keeping columns
c <= r % causal_seq of row r, A = max_c |z_c| over the unmasked part of the
row, u = 2^-8 one round-to-nearest bf16 store and store = u (bf16) or 0 (fp32):

    fwd: |y - ref|  <= (store + (C + 8 + 6 A) 2^-23) ref     masked: exactly 0
    bwd: |dx - ref| <= store |ref|
                       + (C + 4) 2^-23 scale |y| (|dy| + sum_c |dy_c y_c|)

Forward: the row sum of C positive terms is good to (C - 1) 2^-24 relative in
any order; every exp(z - m) has an argument of at most 2 A, so the scale
multiply, the subtraction and the argument scaling inside ``__expf`` each move
it by at most 2 A 2^-24, twice over for numerator and denominator (6 A 2^-23
with room), and the 8 covers the two 1-ulp exp2 results, the reciprocal and
the final multiply. Backward takes the *stored* y: the dot product of C fma
terms errs by C 2^-24 sum|dy y|, the subtraction and two multiplies add
3 2^-24. Nothing here was fitted to a result: the hardware ``__expf`` stays
inside the derived allowance. Worst observed error / bound on an MI355X:
forward 0.994 bf16 / 0.039 fp32, backward 0.993 bf16 / 0.015 fp32 (the bf16
figures are the store term; an honest fp32 emulation on the CPU gives the
same).

x has std 3. In the causal cases the *masked* columns of x hold 1e4 instead:
a kernel may not use them, and one that takes its max over them underflows
every exp to 0. What each (R, C) is for; the route each takes is asserted:

* (7, 64)      wave-per-row kernel (C <= 1024), R no multiple of its 4 rows
               per block
* (5, 100)     odd C
* (9, 504), (9, 252)   just under the bf16 / fp32 vector gate C >= 64 V
* (9, 512), (9, 256), (6, 1024)   vector path of the wave kernel
* (5, 516)     C % 8 != 0: vector for fp32, scalar for bf16
* (3, 1032), (3, 1027)   row-per-block kernel, vector and scalar
* (8195, 64), (2051, 1032)   one row block past the 2048-block grid cap: the
               grid-stride loops make a second trip

The unmarked CPU test runs an fp32 emulation on the same inputs: honest
arithmetic stays within 1.0 of both bounds on every case, and a max taken
over masked columns, a causal mask off by one and a dropped last vector each
exceed 4x. A truncating bf16 store errs by less than 2 u |ref|, so against a
bound that contains u |ref| it can reach 2 and never 4; it is required to
exceed 1.5."""

import functools

import pytest
import torch

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
SCALE = 0.125
U = 2.0 ** -8
KMAXGRID = 2048

# (R, C): (kernel, vector path for bf16, for fp32, second grid-stride trip)
SHAPES = {
    (7, 64): ("wave", False, False, False),
    (5, 100): ("wave", False, False, False),
    (9, 504): ("wave", False, True, False),
    (9, 252): ("wave", False, False, False),
    (9, 512): ("wave", True, True, False),
    (9, 256): ("wave", False, True, False),
    (6, 1024): ("wave", True, True, False),
    (5, 516): ("wave", False, True, False),
    (3, 1032): ("block", True, True, False),
    (3, 1027): ("block", False, False, False),
    (8195, 64): ("wave", False, False, True),
    (2051, 1032): ("block", True, True, True),
}
CASES = [(R, C, dt, causal) for (R, C) in SHAPES for dt in (BF16, FP32)
         for causal in (False, True)]


def case_id(c):
    R, C, dt, causal = c
    return f"{R}x{C}_{'bf16' if dt == BF16 else 'fp32'}" + \
        ("_causal" if causal else "")


def route(R, C, dtype):
    """A model of softmax_route (csrc/attn_route.h), which the launchers
    and kernels execute and tests/test_attention_route.py holds equal to this:
    C <= 1024 picks the wave kernel (4 rows per block), 16-byte vectors need
    C % V == 0 and C >= 64 V, and more than kMaxGrid blocks grid-stride."""
    V = 8 if dtype == BF16 else 4
    wave = C <= 1024
    blocks = (R + 3) // 4 if wave else R
    return ("wave" if wave else "block", C % V == 0 and C >= 64 * V,
            blocks > KMAXGRID)


def check_route(R, C, dtype):
    kernel, vec_bf16, vec_fp32, trip = SHAPES[(R, C)]
    want = (kernel, vec_bf16 if dtype == BF16 else vec_fp32, trip)
    assert route(R, C, dtype) == want, (R, C, dtype, route(R, C, dtype), want)
    if torch.cuda.is_available():   # what the launchers execute
        d = OPS.softmax_route(R, C, dtype == BF16)
        assert (d["kernel"], d["vec"], d["capped"]) == want, (R, C, dtype, d)


def keep_mask(R, C, causal):
    """True where the column is unmasked (causal_seq = C)."""
    if not causal:
        return torch.ones(R, C, dtype=torch.bool)
    qpos = torch.arange(R) % C
    return torch.arange(C)[None, :] <= qpos[:, None]


@functools.lru_cache(maxsize=2)
def inputs(R, C, dtype, causal):
    """Stored x and dy, the float64 forward reference and its bound; never
    modified."""
    g = torch.Generator().manual_seed(7919 * R + C)
    x = torch.randn(R, C, generator=g).mul(3.0)
    dy = torch.randn(R, C, generator=g).to(dtype)
    keep = keep_mask(R, C, causal)
    x = torch.where(keep, x, torch.full_like(x, 1e4)).to(dtype)
    z = (SCALE * x.double()).masked_fill(~keep, float("-inf"))
    ref = torch.softmax(z, dim=-1)
    A = z.masked_fill(~keep, 0.0).abs().amax(dim=-1, keepdim=True)
    store = U if dtype == BF16 else 0.0
    lim = (store + (C + 8 + 6 * A) * 2.0 ** -23) * ref
    return x, dy, keep, ref, lim


def bwd_reference(y, dy, dtype):
    """float64 backward from the stored y, and its bound."""
    C = y.shape[-1]
    yd, dyd = y.double(), dy.double()
    ref = SCALE * yd * (dyd - (dyd * yd).sum(-1, keepdim=True))
    store = U if dtype == BF16 else 0.0
    mag = SCALE * yd.abs() * (dyd.abs() + (dyd * yd).abs().sum(-1, keepdim=True))
    return ref, store * ref.abs() + (C + 4) * 2.0 ** -23 * mag


def worst(got, ref, lim):
    """max error / bound; anything non-finite, or any error where the bound
    is 0, counts as infinite."""
    err = (got.double() - ref).abs()
    r = torch.where(lim > 0, err / lim,
                    torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isfinite(got.double()), r,
                    torch.full_like(r, float("inf")))
    return r.max().item()


# ---- GPU ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_softmax(c):
    R, C, dtype, causal = c
    check_route(R, C, dtype)
    x, dy, keep, ref, lim = inputs(R, C, dtype, causal)
    y = OPS.softmax_fwd(x.to(DEV), SCALE, C if causal else 0)
    assert y.dtype == dtype and tuple(y.shape) == (R, C)
    yc = y.cpu()
    assert (yc[~keep] == 0).all(), "masked columns must be exactly 0"
    rf = worst(yc, ref, lim)
    print(f"softmax_exact {case_id(c)}: fwd worst error / bound = {rf:.4f}")
    dx = OPS.softmax_bwd(y, dy.to(DEV), SCALE)
    assert dx.dtype == dtype and tuple(dx.shape) == (R, C)
    rb = worst(dx.cpu(), *bwd_reference(yc, dy, dtype))
    print(f"softmax_exact {case_id(c)}: bwd worst error / bound = {rb:.4f}")
    assert rf <= 1.0, f"forward error is {rf:.3f} x the bound"
    assert rb <= 1.0, f"backward error is {rb:.3f} x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_softmax_refuses_causal_seq_outside_row(dtype):
    """causal_seq > C would walk c <= r % causal_seq past the row; refused on
    the host, as is a negative one."""
    x = torch.zeros(9, 64, dtype=dtype, device=DEV)
    for bad in (65, 128, -1):
        with pytest.raises(RuntimeError, match="causal_seq"):
            OPS.softmax_fwd(x, SCALE, bad)
    y = OPS.softmax_fwd(x, SCALE, 64)
    assert torch.equal(y[0, :2].float().cpu(), torch.tensor([1.0, 0.0]))


# ---- CPU: the bound admits honest fp32 and rejects single defects -------------

def _store(t, dtype, truncate=False):
    if dtype == FP32:
        return t
    if truncate:
        bits = t.contiguous().view(torch.int32) & -65536
        return bits.view(torch.float32).to(BF16)
    return t.to(BF16)


def emulate_fwd(x, keep, dtype, mutant=None):
    """The kernels' arithmetic in fp32: max and sum over the unmasked part,
    exp(z - m) / sum, one store."""
    R, C = x.shape
    V = 8 if dtype == BF16 else 4
    z = x.float() * SCALE
    if mutant == "causal_off_by_one":
        keep = keep & keep.roll(-1, dims=1)
        keep[:, -1] = False
    cols = C - V if mutant == "dropped_last_vector" else C
    live = keep.clone()
    live[:, cols:] = False
    neg = torch.full_like(z, float("-inf"))
    if mutant == "max_over_masked":
        m = z.amax(dim=-1, keepdim=True)
    else:
        m = torch.where(live, z, neg).amax(dim=-1, keepdim=True)
    e = torch.where(live, torch.exp(z - m), torch.zeros_like(z))
    y = e * (1.0 / e.sum(dim=-1, keepdim=True))
    y = _store(y, dtype, truncate=mutant == "truncating_store")
    if mutant == "dropped_last_vector":
        y[:, cols:] = float("nan")      # never written
    return y


def emulate_bwd(y, dy, dtype, mutant=None):
    R, C = y.shape
    V = 8 if dtype == BF16 else 4
    yf, dyf = y.float(), dy.float()
    cols = C - V if mutant == "dropped_last_vector" else C
    dot = (dyf[:, :cols] * yf[:, :cols]).sum(-1, keepdim=True)
    dx = _store(SCALE * yf * (dyf - dot), dtype,
                truncate=mutant == "truncating_store")
    if mutant == "dropped_last_vector":
        dx[:, cols:] = float("nan")
    return dx


FWD_MUTANTS = ("max_over_masked", "causal_off_by_one", "truncating_store",
               "dropped_last_vector")


def test_bound_admits_fp32_and_rejects_mutants():
    seen = {m: 0.0 for m in FWD_MUTANTS}
    seen_bwd = {"truncating_store": 0.0, "dropped_last_vector": 0.0}
    top_f = top_b = 0.0
    for c in CASES:
        R, C, dtype, causal = c
        check_route(R, C, dtype)
        x, dy, keep, ref, lim = inputs(R, C, dtype, causal)
        y = emulate_fwd(x, keep, dtype)
        assert (y[~keep] == 0).all()
        rf = worst(y, ref, lim)
        bref, blim = bwd_reference(y, dy, dtype)
        rb = worst(emulate_bwd(y, dy, dtype), bref, blim)
        assert rf <= 1.0 and rb <= 1.0, (case_id(c), rf, rb)
        top_f, top_b = max(top_f, rf), max(top_b, rb)
        vec = route(R, C, dtype)[1]
        for m in FWD_MUTANTS:
            if m in ("max_over_masked", "causal_off_by_one") and not causal:
                continue
            if m == "truncating_store" and dtype != BF16:
                continue
            if m == "dropped_last_vector" and not vec:
                continue
            seen[m] = max(seen[m], worst(emulate_fwd(x, keep, dtype, m), ref,
                                         lim))
            if m in seen_bwd:
                seen_bwd[m] = max(seen_bwd[m], worst(
                    emulate_bwd(y, dy, dtype, m), bref, blim))
    print(f"softmax_exact honest fp32: fwd {top_f:.3f}, bwd {top_b:.3f} of "
          f"the bound; mutants fwd {seen}, bwd {seen_bwd}")
    for m, r in seen.items():
        assert r > (1.5 if m == "truncating_store" else 4.0), (m, r)
    assert seen_bwd["truncating_store"] > 1.5, seen_bwd
    assert seen_bwd["dropped_last_vector"] > 4.0, seen_bwd

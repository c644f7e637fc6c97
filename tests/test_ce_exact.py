"""``ce_masked_fwd`` / ``ce_masked_bwd`` (loss.hip, the MASKED instantiations)
in fp32 and bf16 against float64 built from the stored inputs, with bounds
that have no free constants (the form of tests/test_softmax_exact.py), and
bit for bit against the dense ``ce_fwd`` / ``ce_bwd`` on the compacted live
rows.

A row b is live iff 0 <= target[b] < C and target[b] != ignore_index; every
other row is ignored: lse[b] and the whole dx row are +0.0, it adds nothing to
the loss or to n_valid, and its logits are never read. The ignored rows of the
stored logits are NaN, so one read of them poisons the result.

Notation for a live row: x the stored logits, m = max_c x_c (exact),
A = max_c (m - x_c), s = sum_c exp(x_c - m), lse = m + log s, t the label,
r = lse - x_t the row loss, n = n_valid, u = 2^-8 one round-to-nearest bf16
store, store = u (bf16) or 0 (fp32).

    d        = (C + 8 + 6 A) 2^-23                relative error of the sum s
    |lse - ref|  <= -log(1 - d) + 2^-22 log s + 2^-23 |ref|
    |loss - ref| <= mean_b(lse bound of row b) + (n + 2) 2^-24 mean_b |r_b|
    |dx - ref|   <= store |ref| + 2^-22 |ref|
                    + |scale| p (3 |x_c - lse| 2^-24 + 2^-23) + 2^-126

d is the ``__expf``-sum term of test_softmax_exact.py: C positive terms summed
in any order, every exp argument at most A and moved by the subtraction and
the argument scaling inside ``__expf``, 1-ulp exp2 results. A relative error d
of s moves log s by at most -log(1 - d). ``__logf`` is taken as
test_flash_exact.py takes it for its lse, argument rounding plus 1 ulp of the
result: log2 s to 1 ulp and the multiply by the rounded ln 2 make 2^-22 log s,
and 2^-23 |ref| is the final addition m + log s. The loss sums n row losses
with unordered atomics ((n - 1) 2^-24 of the sum of |r_b|), after one
subtraction per row and before one division: (n + 2) 2^-24 mean |r_b|.

The backward is a function of its arguments, so its reference takes the
kernel's own lse: p = exp(x - lse), scale = dout / n, ref = scale (p - onehot).
The exponent x_c - lse is rounded once and scaled inside ``__expf`` (twice
|x_c - lse| 2^-24), the exp2 result is good to 1 ulp; the division dout / n,
the subtraction p - onehot and the multiply by scale are 3 2^-24 |ref|, taken
as 2^-22; 2^-126 covers a result below the smallest normal number. An error of
p next to the label (p - 1 cancels) is absolute and covered by the p term.
Nothing here was fitted to a result; the threshold is 1.0. Worst observed
error / bound on an MI355X over all cases: lse 0.041, loss 0.014, dx 0.995
bf16 (the store term) / 0.598 fp32; the honest fp32 emulation below gives
lse 0.041, loss 0.014, dx 0.995 / 0.553.

dout = 1.7 (as stored in fp32). Logits have std 3, std 8 in one of the BERT
vocabulary cases (A reaches 70, so 6 A counts). The kernels walk a row with 256
threads and run at most kMaxGrid = 2048 blocks. What each case is for:

* (7, 10)       rows 0, 3, 6 ignored (first, middle, last) by the labels C,
                -1 and 2^40 with ignore_index = -100: labels outside [0, C)
                that are not ignore_index are skipped, never read
* (5, 257)      one element into a thread's second trip
* (4, 30528)    the BERT vocabulary, many trips; std 3 and std 8
* (2050, 33)    grid-stride past 2048 blocks: block 0 has row 0 live and row
                2048 ignored, block 1 has row 1 ignored and row 2049 live (a
                skipped row must not unbalance the next row's barriers)
* (6, 64)       ignore_index = 0, a class id in range, labels include 0
* (3, 100)      every row ignored: loss +0.0, n_valid 0, dx +0.0, no NaN
* (8, 1000)     ignore_index = -100 and no row ignored: lse and dx are those
                of ``ce_fwd`` / ``ce_bwd`` bit for bit

The unmarked CPU tests run an fp32 emulation of the two kernels on the same
inputs: honest arithmetic stays within 1.0 of every bound, and each of six
single defects exceeds 4x on a case that reaches it. The CPU fallback of
``cross_entropy(..., ignore_index=k)`` is held to the same contract."""

import functools

import pytest
import torch

from baton_amd.ops import functional as BF

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
U = 2.0 ** -8
DOUT = 1.7
KMAXGRID = 2048
BIG = 2 ** 40


def _labels_small(C):
    return {0: C, 3: -1, 6: BIG}


def _labels_stride(B):
    ign = {b: -100 for b in range(B) if b % 5 == 3}
    ign[1] = -100
    ign[KMAXGRID] = -100            # block 0's second row
    assert 0 not in ign and KMAXGRID + 1 not in ign and B > KMAXGRID + 1
    return ign


# name: (B, C, ignore_index, {ignored row: its label}, std)
SHAPES = {
    "7x10_bad_labels": (7, 10, -100, _labels_small(10), 3.0),
    "5x257": (5, 257, -100, {2: -100}, 3.0),
    "4x30528": (4, 30528, -100, {1: -100}, 3.0),
    "4x30528_std8": (4, 30528, -100, {1: -100, 2: 30528}, 8.0),
    "2050x33_stride": (2050, 33, -100, _labels_stride(2050), 3.0),
    "6x64_ignore0": (6, 64, 0, {1: 0, 4: 0}, 3.0),
    "3x100_all_ignored": (3, 100, -100, {0: -100, 1: -100, 2: -100}, 3.0),
    "8x1000_none_ignored": (8, 1000, -100, {}, 3.0),
}
CASES = [(name, dt) for name in SHAPES for dt in (BF16, FP32)]


def case_id(c):
    return f"{c[0]}_{'bf16' if c[1] == BF16 else 'fp32'}"


def live_rows(t, C, ignore_index):
    return (t >= 0) & (t < C) & (t != ignore_index)


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """Stored logits (NaN in the ignored rows), labels, dout, and the float64
    forward reference with its bounds; never modified."""
    B, C, ignore_index, ignored, std = SHAPES[name]
    g = torch.Generator().manual_seed(104729 * B + C + int(std))
    x = torch.randn(B, C, generator=g).mul(std)
    t = torch.randint(1, C, (B,), generator=g)      # 0 is ignore_index once
    for b, lab in ignored.items():
        t[b] = lab
        x[b] = float("nan")
    x = x.to(dtype)
    live = live_rows(t, C, ignore_index)
    assert sorted(ignored) == (~live).nonzero().flatten().tolist()
    n = int(live.sum())
    xd = x.double()[live]
    m = xd.amax(dim=1)
    A = (m[:, None] - xd).amax(dim=1)
    logs = torch.log(torch.exp(xd - m[:, None]).sum(dim=1))
    lse_live = m + logs
    d = (C + 8 + 6 * A) * 2.0 ** -23
    lim_live = -torch.log1p(-d) + 2.0 ** -22 * logs + 2.0 ** -23 * lse_live.abs()
    r = lse_live - xd.gather(1, t[live][:, None]).squeeze(1)
    lse = torch.zeros(B, dtype=torch.float64)
    lim_lse = torch.zeros(B, dtype=torch.float64)
    lse[live], lim_lse[live] = lse_live, lim_live
    if n:
        loss = r.sum() / n
        lim_loss = lim_live.mean() + (n + 2) * 2.0 ** -24 * r.abs().mean()
    else:
        loss = lim_loss = torch.zeros((), dtype=torch.float64)
    dout = torch.tensor(DOUT, dtype=FP32)
    return dict(x=x, t=t, dout=dout, live=live, n=n, lse=lse, lim_lse=lim_lse,
                loss=loss, lim_loss=lim_loss, ignore_index=ignore_index)


def bwd_reference(f, lse, dtype):
    """float64 dx from the given lse, and its bound; both 0 on ignored rows."""
    x, t, live, n = f["x"], f["t"], f["live"], f["n"]
    B, C = x.shape
    ref = torch.zeros(B, C, dtype=torch.float64)
    lim = torch.zeros(B, C, dtype=torch.float64)
    if n == 0:
        return ref, lim
    scale = f["dout"].double() / n
    arg = x.double()[live] - lse.double()[live][:, None]
    p = torch.exp(arg)
    one = torch.zeros_like(p)
    one.scatter_(1, t[live][:, None], 1.0)
    r = scale * (p - one)
    store = U if dtype == BF16 else 0.0
    ref[live] = r
    lim[live] = (store * r.abs() + 2.0 ** -22 * r.abs() + scale.abs() * p
                 * (3 * arg.abs() * 2.0 ** -24 + 2.0 ** -23) + 2.0 ** -126)
    return ref, lim


def worst(got, ref, lim):
    """max error / bound; anything non-finite, or any error where the bound
    is 0, counts as infinite."""
    got = got.double()
    err = (got - ref).abs()
    r = torch.where(lim > 0, err / lim,
                    torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return r.max().item()


def is_pos_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == FP32 else torch.int16)


def ratios(f, dtype, loss, lse, dx):
    rb, lb = bwd_reference(f, lse, dtype)
    return (worst(lse, f["lse"], f["lim_lse"]),
            worst(loss.reshape(()), f["loss"], f["lim_loss"]),
            worst(dx, rb, lb))


# ---- GPU ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_ce_masked(c):
    name, dtype = c
    f = inputs(name, dtype)
    B, C = f["x"].shape
    live, n, ign = f["live"], f["n"], f["ignore_index"]
    x, t, dout = f["x"].to(DEV), f["t"].to(DEV), f["dout"].to(DEV)
    loss, lse, n_valid = OPS.ce_masked_fwd(x, t, ign)
    assert loss.dtype == FP32 and loss.dim() == 0
    assert lse.dtype == FP32 and tuple(lse.shape) == (B,)
    assert n_valid.dtype == torch.int32 and n_valid.numel() == 1
    dx = OPS.ce_masked_bwd(x, t, lse, n_valid, dout, ign)
    assert dx.dtype == dtype and tuple(dx.shape) == (B, C)
    loss_c, lse_c, dx_c = loss.cpu(), lse.cpu(), dx.cpu()
    assert n_valid.item() == n
    assert is_pos_zero(lse_c[~live]), "lse of an ignored row must be +0.0"
    assert is_pos_zero(dx_c[~live]), "dx of an ignored row must be +0.0"
    if n:
        # same per-row arithmetic and the same dout / (float)n as the dense
        # kernels on the live rows alone
        xl, tl = x[live.to(DEV)].contiguous(), t[live.to(DEV)].contiguous()
        _, lse_d = OPS.ce_fwd(xl, tl)
        dx_d = OPS.ce_bwd(xl, tl, lse_d, dout)
        assert torch.equal(bits(lse_c[live]), bits(lse_d.cpu()))
        assert torch.equal(bits(dx_c[live]), bits(dx_d.cpu()))
    else:
        assert is_pos_zero(loss_c.reshape(1)), "no live row: loss must be +0.0"
    r_lse, r_loss, r_dx = ratios(f, dtype, loss_c, lse_c, dx_c)
    print(f"ce_exact {case_id(c)}: worst error / bound lse {r_lse:.4f} "
          f"loss {r_loss:.4f} dx {r_dx:.4f}")
    assert r_lse <= 1.0, f"lse error is {r_lse:.3f} x the bound"
    assert r_loss <= 1.0, f"loss error is {r_loss:.3f} x the bound"
    assert r_dx <= 1.0, f"dx error is {r_dx:.3f} x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32])
def test_cross_entropy_autograd_routes_to_masked(dtype):
    """``cross_entropy(..., ignore_index=k)`` on the GPU is the two masked ops:
    same loss bits, and the gradient of 1.7 * loss is ce_masked_bwd's dx."""
    f = inputs("7x10_bad_labels", dtype)
    x = f["x"].to(DEV).requires_grad_(True)
    t = f["t"].to(DEV)
    loss = BF.cross_entropy(x, t, ignore_index=-100)
    (loss * f["dout"].to(DEV)).backward()
    l2, lse, nv = OPS.ce_masked_fwd(x.detach(), t, -100)
    dx = OPS.ce_masked_bwd(x.detach(), t, lse, nv, f["dout"].to(DEV), -100)
    assert torch.equal(bits(x.grad), bits(dx))
    # the row atomics are unordered: the loss is held to its bound, not to bits
    assert worst(loss.detach().cpu().reshape(()), f["loss"],
                 f["lim_loss"]) <= 1.0
    assert worst(l2.cpu().reshape(()), f["loss"], f["lim_loss"]) <= 1.0


def _allocations():
    return torch.cuda.memory_stats(DEV).get("allocation.all.allocated", 0)


def _refused(match, fn):
    before = _allocations()
    with pytest.raises(RuntimeError, match=match):
        fn()
    assert _allocations() == before, "a refusal must come before any allocation"


def _valid(dtype=BF16, B=6, C=40):
    x = torch.zeros(B, C, dtype=dtype, device=DEV)
    t = torch.arange(B, device=DEV)
    return dict(x=x, t=t, lse=torch.zeros(B, device=DEV),
                nv=torch.full((1,), B, dtype=torch.int32, device=DEV),
                dout=torch.ones((), device=DEV))


def _fwd(a):
    return OPS.ce_masked_fwd(a["x"], a["t"], -100)


def _bwd(a):
    return OPS.ce_masked_bwd(a["x"], a["t"], a["lse"], a["nv"], a["dout"], -100)


@pytest.mark.gpu
def test_refuses_bad_logits_and_target():
    """Refused on the host by argument name, before anything is allocated, by
    the forward and by the backward."""
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    bad = {
        "logits_cpu": ("x", torch.zeros(6, 40), "logits"),
        "logits_3d": ("x", z(2, 3, 40), "logits"),
        "logits_1d": ("x", z(6), "logits"),
        "logits_transposed": ("x", z(40, 6).t(), "logits"),
        "logits_fp16": ("x", z(6, 40, dtype=torch.float16), "logits"),
        "logits_fp64": ("x", z(6, 40, dtype=torch.float64), "logits"),
        "logits_B0": ("x", z(0, 40), "logits"),
        "logits_C0": ("x", z(6, 0), "logits"),
        "target_int32": ("t", z(6, dtype=torch.int32), "target"),
        "target_strided": ("t", z(12, dtype=torch.int64)[::2], "target"),
        "target_cpu": ("t", torch.zeros(6, dtype=torch.int64), "target"),
        "target_short": ("t", z(5, dtype=torch.int64), "target"),
        "target_long": ("t", z(7, dtype=torch.int64), "target"),
    }
    for key, (arg, val, match) in bad.items():
        a = _valid()
        a[arg] = val
        _refused(match, lambda: _fwd(a))
        _refused(match, lambda: _bwd(a))
    a = _valid()
    _fwd(a)
    _bwd(a)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2 ** 31, 1), (1, 2 ** 31)],
                         ids=["B_beyond_int", "C_beyond_int"])
def test_refuses_sizes_beyond_int(shape):
    """B or C that does not fit the kernels' int index: 4 GiB of uninitialized
    bf16 that nothing reads."""
    a = _valid()
    a["x"] = torch.empty(shape, dtype=BF16, device=DEV)
    _refused("logits", lambda: _fwd(a))
    _refused("logits", lambda: _bwd(a))
    del a
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_refuses_bad_backward_arguments():
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    bad = {
        "lse_bf16": ("lse", z(6, dtype=BF16), "lse"),
        "lse_short": ("lse", z(5), "lse"),
        "lse_2d": ("lse", z(6, 1), "lse"),
        "lse_strided": ("lse", z(12)[::2], "lse"),
        "lse_cpu": ("lse", torch.zeros(6), "lse"),
        "n_valid_int64": ("nv", z(1, dtype=torch.int64), "n_valid"),
        "n_valid_fp32": ("nv", z(1), "n_valid"),
        "n_valid_two": ("nv", z(2, dtype=torch.int32), "n_valid"),
        "n_valid_cpu": ("nv", torch.zeros(1, dtype=torch.int32), "n_valid"),
        "dout_bf16": ("dout", z((), dtype=BF16), "dout"),
        "dout_vector": ("dout", z(6), "dout"),
        "dout_cpu": ("dout", torch.ones(()), "dout"),
    }
    for key, (arg, val, match) in bad.items():
        a = _valid()
        a[arg] = val
        _refused(match, lambda: _bwd(a))
    _bwd(_valid())


# ---- CPU: the bounds admit honest fp32 and reject single defects --------------

MUTANTS = ("divide_by_B", "ignored_row_in_loss", "ignored_dx_scale_p",
           "n_valid_counts_ignored", "label_of_next_row",
           "ignore_index_scored")


def emulate(f, dtype, mutant=None):
    """The two MASKED kernels' arithmetic in fp32: per live row m, sum of
    exp(x - m), lse = m + log(sum), loss_sum += lse - x_t, n_valid += 1;
    loss = loss_sum / n; dx = (dout / n) (exp(x - lse) - onehot), one store.
    Returns (loss, lse, n_valid, dx)."""
    x, t, ign = f["x"].float(), f["t"], f["ignore_index"]
    B, C = x.shape
    if mutant == "label_of_next_row":
        t = t.roll(-1)
    live = (t >= 0) & (t < C)
    if mutant != "ignore_index_scored":
        live &= t != ign
    tc = t.clamp(0, C - 1)
    m = x.amax(dim=1)
    lse_all = m + torch.log(torch.exp(x - m[:, None]).sum(dim=1))
    row_all = lse_all - x.gather(1, tc[:, None]).squeeze(1)
    zero = torch.zeros(B)
    lse = torch.where(live, lse_all, zero)
    scored = torch.ones_like(live) if mutant == "ignored_row_in_loss" else live
    loss_sum = torch.where(scored, row_all, zero).sum()
    n = B if mutant == "n_valid_counts_ignored" else int(live.sum())
    div = B if mutant == "divide_by_B" else n
    if div > 0:
        loss = loss_sum / torch.tensor(float(div))
        scale = f["dout"] / torch.tensor(float(div))
    else:
        loss, scale = torch.zeros(()), torch.zeros(())
    p = torch.exp(x - lse_all[:, None])
    one = torch.zeros(B, C).scatter_(1, tc[:, None], 1.0)
    dx = torch.where(live[:, None], scale * (p - one), torch.zeros(()))
    if mutant == "ignored_dx_scale_p":
        dx = torch.where(live[:, None], dx, scale * p)
    return loss, lse, n, dx.to(dtype)


def score(f, dtype, out):
    """Worst ratio over lse, loss and dx; a wrong n_valid is infinite."""
    loss, lse, n, dx = out
    if n != f["n"]:
        return float("inf")
    return max(ratios(f, dtype, loss, lse, dx))


def test_bounds_admit_fp32_and_reject_mutants():
    top = [0.0, 0.0, 0.0, 0.0]      # lse, loss, dx bf16, dx fp32
    seen = {m: 0.0 for m in MUTANTS}
    for c in CASES:
        name, dtype = c
        f = inputs(name, dtype)
        loss, lse, n, dx = emulate(f, dtype)
        assert n == f["n"]
        assert is_pos_zero(lse[~f["live"]]) and is_pos_zero(dx[~f["live"]])
        r = ratios(f, dtype, loss, lse, dx)
        assert max(r) <= 1.0, (case_id(c), r)
        top[0], top[1] = max(top[0], r[0]), max(top[1], r[1])
        k = 2 if dtype == BF16 else 3
        top[k] = max(top[k], r[2])
        for m in MUTANTS:
            seen[m] = max(seen[m], score(f, dtype, emulate(f, dtype, m)))
    print(f"ce_exact honest fp32: lse {top[0]:.3f} loss {top[1]:.3f} "
          f"dx bf16 {top[2]:.3f} fp32 {top[3]:.3f}; mutants {seen}")
    for m, r in seen.items():
        assert r > 4.0, (m, r)


def test_mutants_reach_their_case():
    """Each defect on the one case built for it, without the NaN poison doing
    the work where a finite figure exists: the divisor and the count on
    (7, 10), the neighbour's label with no row ignored, the in-range
    ignore_index on (6, 64)."""
    f = inputs("7x10_bad_labels", FP32)
    assert score(f, FP32, emulate(f, FP32, "divide_by_B")) > 4.0
    loss, _, n, _ = emulate(f, FP32, "n_valid_counts_ignored")
    assert n == 7 != f["n"]
    f = inputs("8x1000_none_ignored", FP32)
    s = score(f, FP32, emulate(f, FP32, "label_of_next_row"))
    assert 4.0 < s < float("inf")
    assert score(f, FP32, emulate(f, FP32, "divide_by_B")) <= 1.0   # n == B
    f = inputs("6x64_ignore0", FP32)
    assert emulate(f, FP32, "ignore_index_scored")[2] == 6 != f["n"]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cpu_fallback_contract(c):
    """``cross_entropy(..., ignore_index=k)`` without a GPU: the live-row
    rule, the mean over live rows, 0 when there are none, zero rows in dx.
    The fallback keeps no lse, so the dx reference takes the float64 one and
    the bound gains |scale| p times the lse bound."""
    name, dtype = c
    f = inputs(name, dtype)
    x = f["x"].clone().requires_grad_(True)
    loss = BF.cross_entropy(x, f["t"], ignore_index=f["ignore_index"])
    (loss * f["dout"]).backward()
    live, n = f["live"], f["n"]
    assert x.grad.dtype == dtype
    assert bool((x.grad[~live] == 0).all())
    assert worst(loss.detach().reshape(()), f["loss"], f["lim_loss"]) <= 1.0
    ref, lim = bwd_reference(f, f["lse"], dtype)
    if n:
        p = torch.exp(f["x"].double()[live] - f["lse"][live][:, None])
        lim[live] += (f["dout"].double() / n) * p * f["lim_lse"][live][:, None]
    else:
        assert loss.item() == 0.0 and bool((x.grad == 0).all())
    assert worst(x.grad, ref, lim) <= 1.0


def test_cpu_dense_path_is_untouched():
    """ignore_index=None is the dense loss: the mean over B."""
    f = inputs("8x1000_none_ignored", FP32)
    a = BF.cross_entropy(f["x"], f["t"])
    b = BF.cross_entropy(f["x"], f["t"], ignore_index=None)
    c = BF.cross_entropy(f["x"], f["t"], ignore_index=-100)
    assert torch.equal(a, b)
    assert abs(a.item() - c.item()) <= 2 * f["lim_loss"].item()

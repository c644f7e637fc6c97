"""Global grad-norm clipping, the non-finite step skip and decoupled weight
decay of the fused optimizers (optim.hip: grad_sumsq_kernel,
clip_finalize_kernel, the EXT instantiations of sgd_kernel / adam_kernel;
ops/optim.py: ``max_grad_norm`` / ``decoupled_weight_decay``).

Notation: e = 2^-24 (one fp32 rounding), u = 2^-8 for a bf16 store (the bound
the SGD check is given; a round-to-nearest store needs half of it, the other
half carries the last fma's e |p|) and u = 2^-23 for an fp32 store (the last
fma's rounding and, with decoupled decay, the decay fma's).

The norm. grad_sumsq_kernel runs the step kernels' grid
G = min(2048, ceil((n / 8 + 1) / 256)) blocks of 256 threads. With V elements
per 16-byte vector (8 bf16, 4 fp32), thread i chains acc = fma(x, x, acc) in
fp32 over vectors i, i + 256 G, ... of the n / V whole vectors, element by
element, and then over tail element (n / V) V + i if that is below n: a chain
of T = ceil((n / V) / (256 G)) V + (1 if n % V else 0) roundings at most (the
square itself is not rounded inside the fma). The wave reduction adds 6
shuffle levels, the block adds the 4 wave sums in order to 0.0f (4 adds, the
first exact). All terms are non-negative, so whatever the order the relative
error of a block's partial is at most (T + 10) e; the fp64 finalize (a chain
of ceil(count / 256) adds and 8 tree levels, 2^-53 each) and its fp64 sqrt
add nothing visible. The square root halves the relative error and the store
of the norm rounds once more, e. With the two roundings of slack the issue
allows for a separately rounded square:

    |norm / ref - 1| <= (T + 12) 2^-25 + 2^-23
    |coef / ref - 1| <= 2^-22

the coef against min(1, max_norm / (norm + 1e-6)) recomputed in float64 from
the STORED fp32 norm: the kernel divides by the unrounded norm (e) and rounds
the quotient (e).

The step. With g' = fl(coef g), the SGD kernel computes
grad = fma(wd, p0, g'), mom = fma(mu, m0, grad), p = fma(-lr, mom, p0) and
stores p: three roundings in front of the last fma, each of a quantity that
|coef g| + wd |p0| + mu |m0| bounds:

    |p - ref| <= u |ref| + 3 e lr (|coef g| + wd |p0| + mu |m0|)          (SGD)

Adam (b1, b2 the fp32 betas, s = lr / bc1, r = 1 / sqrt(bc2), both rounded to
fp32 by the binding and taken from there by the reference) continues the same
chain. grad carries dG = 2 e (|coef g| + wd |p0|) (the multiply and the fma).
m = fma(b1, m0, fl(fl(1 - b1) grad)) adds three roundings, v =
fma(b2, v0, fl(fl(fl(1 - b2) grad) grad)) four:

    dm = (1 - b1) dG + 3 e ((1 - b1) |grad| + b1 |m0|)
    dv = 2 (1 - b2) |grad| dG + 4 e ((1 - b2) grad^2 + b2 v0)

denom = fma(sqrt(v), r, eps): the square root halves dv / v and rounds once
(e, correctly rounded), the fma once more, r was rounded once: relative error
at most rd = dv / (2 v) + 3 e. The quotient m / denom rounds once (the
division, correctly rounded, e) and the step size fl(-lr s) carries the
roundings of s and of the product (2 e), with one more e of slack:

    dupd = (s lr / denom) (dm + |m| (rd + 4 e))
    |p - ref| <= u |ref| + (1 + 2^-10) dupd [+ 3 e lr wd |p0|]          (Adam)

(1 + 2^-10) covers the second-order terms. The bracket is the decoupled
decay: p' = fma(fl(-lr wd), p0, p0), whose factor carries the product's
rounding (e; lr and wd are fp32 inputs) and two of slack; the rounding of p'
itself is in u |ref|. The decoupled reference is torch.optim.AdamW's update
p0 (1 - lr wd) - upd with no L2 term in grad.

Wherever the bound is not needed the check is for bits: an EXT step with
coef == 1.0f against the dense op, an fp32 EXT step against the dense op fed
torch's fp32 coef * g, a skipped step against the untouched inputs, a graph
replay against the eager optimizer.

The step checks run at n = 10007 and, in the *_flat_sizes tests, over
step_sizes(V): n in {1, V - 1, V, V + 1, 255 V + 3, 256 V + 1, 4194333}, the
flat shapes of the other exact tests: nothing but a tail, exactly one vector,
a vector and a tail, one block with a partly filled last wave, two blocks, and
a size past the capped grid (2048 blocks of 256 threads), where a thread takes
a second vector and there is a tail. The bounds are per element, so they do
not depend on n.

The unmarked emulation test runs the same arithmetic in numpy (fp32 chains,
the 6 shuffle levels, the 4 waves, the fp64 finalize, the fp32 SGD and Adam
steps) over the same sizes: honest arithmetic stays within 1.0 of every bound
on every case, and each single defect exceeds 4x on the input chosen for it.

Figures measured on an MI355X (records, not thresholds) are in
profiles/r09_grad_clip.md."""

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from baton_amd.ops.optim import FusedAdam, FusedSGD, make_optimizer
from baton_amd.runtime.arena import FlatParamArena
from baton_amd.utils.config import BatonConfig, TrainConfig

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

E = 2.0 ** -24
KBLOCK, KMAXGRID = 256, 2048
VEC = {torch.float32: 4, torch.bfloat16: 8}


def grid_of(n):
    return min(KMAXGRID, max(1, -(-(n // 8 + 1) // KBLOCK)))


def chain_of(n, V):
    """T: the elements one thread accumulates at most."""
    G = grid_of(n)
    return -(-(n // V) // (KBLOCK * G)) * V + (1 if n % V else 0)


def norm_bound(T):
    return (T + 12) * 2.0 ** -25 + 2.0 ** -23


COEF_BOUND = 2.0 ** -22


def norm_sizes(V):
    return [1, V - 1, V, 256 * V, 256 * V + 1, 10007, 2048 * 256 * V + V + 1]


def step_sizes(V):
    return [1, V - 1, V, V + 1, 255 * V + 3, 256 * V + 1, 4194333]


@functools.lru_cache(maxsize=None)
def make_input(n, dtype, scale=1.0):
    """Unit-variance data (times scale) on the CPU, |x| = 16 scale planted at
    the last element (the tail's, if there is one) and in the last whole
    vector, where an indexing defect would lose it. Shared; never modified."""
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    V = VEC[dtype]
    x[n - 1] = 16.0
    if n >= V:
        x[(n // V) * V - 1] = -16.0
    return (x * scale).to(dtype)


def ref_norm(*xs):
    return math.sqrt(sum(float(x.double().pow(2).sum()) for x in xs))


def ref_coef(norm32, max_norm):
    return min(1.0, max_norm / (float(norm32) + 1e-6))


# ---- fp32 emulation of the kernels (numpy) ----------------------------------

def f32(x):
    return np.asarray(x, dtype=np.float32)


def fma32(a, b, c):
    a, b, c = (np.asarray(t, np.float64) for t in (a, b, c))
    return (a * b + c).astype(np.float32)


def bf16_round(x):
    u = f32(x).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def emu_partials(x, V, drop_tail=False):
    """grad_sumsq_kernel: one fp32 partial per block."""
    x = f32(x)
    n = x.size
    G = grid_of(n)
    nthr = G * KBLOCK
    nvec = n // V
    trips = -(-nvec // nthr)
    # [thread, trip, V]: zeros where a thread has no vector (fma(0, 0, acc)
    # is acc exactly)
    body = np.zeros(trips * nthr * V, np.float32)
    body[: nvec * V] = x[: nvec * V]
    body = body.reshape(trips, nthr, V).transpose(1, 0, 2).reshape(
        nthr, trips * V)
    acc = np.zeros(nthr, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(body.shape[1]):
            acc = fma32(body[:, k], body[:, k], acc)
        if not drop_tail and n > nvec * V:
            tail = np.zeros(nthr, np.float32)
            tail[: n - nvec * V] = x[nvec * V:]
            acc = fma32(tail, tail, acc)
        v = acc.reshape(-1, 64)
        for off in (32, 16, 8, 4, 2, 1):        # __shfl_down levels
            w = v.copy()
            w[:, : 64 - off] = v[:, : 64 - off] + v[:, off:]
            v = w
        waves = v[:, 0].reshape(G, KBLOCK // 64)
        total = np.zeros(G, np.float32)
        for i in range(KBLOCK // 64):
            total = total + waves[:, i]
    return total


def emu_finalize(partials, max_norm, skipped=0.0, drop_last=False,
                 no_sqrt=False, no_min=False):
    """clip_finalize_kernel -> clip_state as 4 fp32."""
    p = np.concatenate(partials).astype(np.float64)
    if drop_last:
        p = p[:-1]
    red = np.zeros(KBLOCK, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(min(KBLOCK, p.size)):
            acc = 0.0
            for v in p[t::KBLOCK]:
                acc += v
            red[t] = acc
        w = KBLOCK // 2
        while w:
            red[:w] = red[:w] + red[w:2 * w]
            w //= 2
        sumsq = red[0]
        finite = bool(np.isfinite(sumsq))
        norm = sumsq if no_sqrt else np.sqrt(sumsq)
        c = max_norm / (norm + 1e-6)
        if not no_min:
            c = min(1.0, c)
        return f32([norm, c if finite else 0.0, 1.0 if finite else 0.0,
                    skipped if finite else skipped + 1.0])


def emu_sgd(p0, g, m0, lr, mu, wd, state, bf16, coef_after_wd=False,
            skip_writes_m=False):
    """sgd_kernel<T, EXT> with momentum, L2 decay; returns (p, m)."""
    p0, g, m0 = f32(p0), f32(g), f32(m0)
    lr, mu, wd = np.float32(lr), np.float32(mu), np.float32(wd)
    with np.errstate(over="ignore", invalid="ignore"):
        if state[2] == 0.0:
            if skip_writes_m:
                return p0, fma32(mu, m0, g)
            return p0, m0
        coef = state[1]
        if coef_after_wd:
            grad = coef * fma32(wd, p0, g)
        else:
            grad = fma32(wd, p0, coef * g)
        mom = fma32(mu, m0, grad)
        p = fma32(-lr, mom, p0)
    return (bf16_round(p) if bf16 else p), mom


def emu_adam(p0, g, m0, v0, lr, b1, b2, eps, wd, bc1, bc2, coef, bf16,
             decoupled):
    """adam_kernel<T, EXT> on a finite step; returns p."""
    p0, g, m0, v0 = f32(p0), f32(g), f32(m0), f32(v0)
    lr, b1, b2, eps, wd = (np.float32(a) for a in (lr, b1, b2, eps, wd))
    s = np.float32(1.0 / bc1)
    r = np.float32(1.0 / math.sqrt(bc2))
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        gc = np.float32(coef) * g
        if decoupled:
            p0 = fma32(-lr * wd, p0, p0)
            grad = gc
        else:
            grad = fma32(wd, p0, gc)
        m = fma32(b1, m0, (one - b1) * grad)
        v = fma32(b2, v0, (one - b2) * grad * grad)
        denom = fma32(np.sqrt(v), r, eps)
        p = fma32(-lr * s, m / denom, p0)
    return bf16_round(p) if bf16 else p


def sgd_ratio(p, p0, g, m0, lr, mu, wd, coef, u):
    """max |p - ref| / bound of the SGD step against float64."""
    p0, g, m0 = (np.asarray(a, np.float64) for a in (p0, g, m0))
    lr, mu, wd = (float(np.float32(a)) for a in (lr, mu, wd))
    cg = float(coef) * g
    ref = p0 - lr * (mu * m0 + cg + wd * p0)
    bound = u * np.abs(ref) + 3 * E * lr * (np.abs(cg) + wd * np.abs(p0)
                                            + mu * np.abs(m0))
    return float(np.max(np.abs(np.float64(p) - ref) / bound))


def adam_ratio(p, p0, g, m0, v0, lr, b1, b2, eps, wd, bc1, bc2, coef, u,
               decoupled):
    """max |p - ref| / bound of the Adam / AdamW step (module docstring)."""
    p0, g, m0, v0 = (np.asarray(a, np.float64) for a in (p0, g, m0, v0))
    lr, b1, b2, eps, wd = (float(np.float32(a)) for a in (lr, b1, b2, eps, wd))
    s = float(np.float32(1.0 / bc1))
    r = float(np.float32(1.0 / math.sqrt(bc2)))
    cg = float(coef) * g
    wl2 = 0.0 if decoupled else wd
    grad = cg + wl2 * p0
    dG = 2 * E * (np.abs(cg) + wl2 * np.abs(p0))
    m = b1 * m0 + (1 - b1) * grad
    v = b2 * v0 + (1 - b2) * grad * grad
    dm = (1 - b1) * dG + 3 * E * ((1 - b1) * np.abs(grad) + b1 * np.abs(m0))
    dv = 2 * (1 - b2) * np.abs(grad) * dG + 4 * E * ((1 - b2) * grad * grad
                                                    + b2 * v0)
    denom = np.sqrt(v) * r + eps
    rd = dv / (2 * v) + 3 * E
    dupd = s * lr / denom * (dm + np.abs(m) * (rd + 4 * E))
    pd = p0 * (1 - lr * wd) if decoupled else p0
    ref = pd - lr * s * m / denom
    bound = u * np.abs(ref) + (1 + 2.0 ** -10) * dupd
    if decoupled:
        bound = bound + 3 * E * lr * wd * np.abs(p0)
    return float(np.max(np.abs(np.float64(p) - ref) / bound))


def _emu_norm_ratios(xs, Vs, max_norm, **mut):
    """(norm ratio, coef ratio, state) of the emulated two-stage reduction
    over the groups xs against float64; mut: the defects."""
    drop_tail = mut.pop("drop_tail", False)
    omit_group = mut.pop("omit_group", False)
    parts = [emu_partials(x.float().numpy(), V, drop_tail)
             for x, V in zip(xs, Vs)]
    if omit_group:
        parts = parts[:-1]
    st = emu_finalize(parts, max_norm, **mut)
    T = max(chain_of(x.numel(), V) for x, V in zip(xs, Vs))
    ref = ref_norm(*xs)
    rn = abs(float(st[0]) / ref - 1.0) / norm_bound(T) if ref > 0 else float(
        st[0] != 0.0)
    rc = abs(float(st[1]) / ref_coef(st[0], max_norm) - 1.0) / COEF_BOUND
    return rn, rc, st


def test_emulated_reduction_meets_the_bounds():
    worst_n = worst_c = 0.0
    for dtype, V in ((torch.float32, 4), (torch.bfloat16, 8)):
        for n in norm_sizes(V):
            x = make_input(n, dtype)
            nrm = ref_norm(x)
            for max_norm in (2.0 * nrm, 0.5 * nrm, math.inf):
                rn, rc, st = _emu_norm_ratios([x], [V], max_norm)
                print(f"emu {dtype} n={n} max/norm={max_norm / nrm:.1f}: "
                      f"norm {rn:.3f} coef {rc:.3f}")
                worst_n, worst_c = max(worst_n, rn), max(worst_c, rc)
                assert rn <= 1.0 and rc <= 1.0
                if max_norm > nrm:
                    assert st[1] == np.float32(1.0)
                assert st[2] == 1.0 and st[3] == 0.0
    # two groups, one norm
    xs = [make_input(10007, torch.bfloat16), make_input(1025, torch.float32)]
    rn, rc, _ = _emu_norm_ratios(xs, [8, 4], 0.5 * ref_norm(*xs))
    assert rn <= 1.0 and rc <= 1.0
    # zeros: norm 0, coef 1
    st = emu_finalize([emu_partials(np.zeros(1000, np.float32), 4)], 1.0)
    assert st.tolist() == [0.0, 1.0, 1.0, 0.0]
    print(f"emu worst: norm {worst_n:.3f} coef {worst_c:.3f}")


@functools.lru_cache(maxsize=None)
def _step_case(dtype, n=1031):
    """(p0, g, m0, v0) as fp32 numpy arrays. Shared; never modified."""
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen).to(dtype).float().numpy()
    g = make_input(n, dtype).float().numpy()
    m0 = torch.randn(n, generator=gen).numpy()
    v0 = (torch.rand(n, generator=gen) + 0.5).numpy()
    return p0, g, m0, v0


def test_emulated_step_meets_the_bound():
    lr, mu, wd = 0.1, 0.9, 0.1
    h = ADAM_HP
    worst = 0.0
    for bf16, u in ((False, 2.0 ** -23), (True, 2.0 ** -8)):
        dtype = torch.bfloat16 if bf16 else torch.float32
        for n in [1031] + step_sizes(VEC[dtype]):
            p0, g, m0, v0 = _step_case(dtype, n)
            x = torch.from_numpy(g)
            st = emu_finalize([emu_partials(g, VEC[dtype])],
                              0.5 * ref_norm(x))
            assert 0.4 < st[1] < 0.6
            p, m = emu_sgd(p0, g, m0, lr, mu, wd, st, bf16)
            rs = [sgd_ratio(p, p0, g, m0, lr, mu, wd, st[1], u)]
            for decoupled in (False, True):
                p = emu_adam(p0, g, m0, v0, h["lr"], h["beta1"], h["beta2"],
                             h["eps"], h["weight_decay"], h["bc1"], h["bc2"],
                             st[1], bf16, decoupled)
                rs.append(adam_ratio(p, p0, g, m0, v0, h["lr"], h["beta1"],
                                     h["beta2"], h["eps"], h["weight_decay"],
                                     h["bc1"], h["bc2"], st[1], u, decoupled))
            print(f"emu bf16={bf16} n={n}: sgd {rs[0]:.3f} adam {rs[1]:.3f} "
                  f"adamw {rs[2]:.3f}")
            worst = max(worst, *rs)
            assert max(rs) <= 1.0
    print(f"emu step worst: {worst:.3f}")


def test_single_defects_exceed_4x():
    V, dtype = 8, torch.bfloat16
    x = make_input(256 * V + 1, dtype)
    # a dropped scalar tail: the planted last element is the tail
    assert _emu_norm_ratios([x], [V], math.inf, drop_tail=True)[0] > 4.0
    # a dropped last block's partial: 5 blocks at n = 10007
    x = make_input(10007, dtype)
    assert grid_of(10007) == 5
    assert _emu_norm_ratios([x], [V], math.inf, drop_last=True)[0] > 4.0
    # an omitted group
    xs = [x, make_input(1025, torch.float32)]
    assert _emu_norm_ratios(xs, [8, 4], math.inf, omit_group=True)[0] > 4.0
    # a missing sqrt
    assert _emu_norm_ratios([x], [V], math.inf, no_sqrt=True)[0] > 4.0
    # a clip applied although norm < max_norm: coef must be exactly 1
    nrm = ref_norm(x)
    rn, rc, st = _emu_norm_ratios([x], [V], 2.0 * nrm, no_min=True)
    assert rn <= 1.0 and rc > 4.0 and st[1] != np.float32(1.0)
    # coef applied after the weight decay (fp32: the sharpest bound)
    lr, mu, wd = 0.1, 0.9, 0.1
    p0, g, m0, _ = _step_case(torch.float32)
    st = emu_finalize([emu_partials(g, 4)], 0.5 * ref_norm(torch.from_numpy(g)))
    p, _ = emu_sgd(p0, g, m0, lr, mu, wd, st, False, coef_after_wd=True)
    assert sgd_ratio(p, p0, g, m0, lr, mu, wd, st[1], 2.0 ** -23) > 4.0
    # a skipped step that still writes m: the check is for bits
    gi = g.copy()
    gi[-1] = np.inf
    st = emu_finalize([emu_partials(gi, 4)], 1.0, skipped=2.0)
    assert st.tolist() == [np.inf, 0.0, 0.0, 3.0]
    p, m = emu_sgd(p0, gi, m0, lr, mu, wd, st, False)
    assert np.array_equal(p.view(np.int32), p0.view(np.int32))
    assert np.array_equal(m.view(np.int32), m0.view(np.int32))
    p, m = emu_sgd(p0, gi, m0, lr, mu, wd, st, False, skip_writes_m=True)
    assert not np.array_equal(m.view(np.int32), m0.view(np.int32))


# ---- CPU fallback against torch ---------------------------------------------

def _two_tensor_model():
    torch.manual_seed(3)
    return [nn.Parameter(torch.randn(5, 3)), nn.Parameter(torch.randn(7))]


def _grads_for(params, step, target_norm):
    gen = torch.Generator().manual_seed(100 + step)
    gs = [torch.randn(p.shape, generator=gen) for p in params]
    nrm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs))
    return [g * (target_norm / nrm) for g in gs]


def _make(kind, params, max_grad_norm):
    if kind == "sgd":
        return FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=0.01,
                        max_grad_norm=max_grad_norm)
    if kind == "adam":
        return FusedAdam(params, lr=0.01, weight_decay=0.01,
                         max_grad_norm=max_grad_norm)
    cfg = TrainConfig(optimizer="adamw", lr=0.01, weight_decay=0.01,
                      max_grad_norm=max_grad_norm or 0.0)
    return make_optimizer(params, cfg)


def _make_torch(kind, params):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=0.01)
    if kind == "adam":
        return torch.optim.Adam(params, lr=0.01, weight_decay=0.01)
    return torch.optim.AdamW(params, lr=0.01, weight_decay=0.01)


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("rel_norm", [0.5, 2.0])
def test_fallback_follows_torch(kind, rel_norm):
    ours, theirs, plain = (_two_tensor_model() for _ in range(3))
    o = _make(kind, ours, 1.0)
    t = _make_torch(kind, theirs)
    u = _make(kind, plain, None)       # the unclipped optimizer
    assert o.decoupled_weight_decay == (kind == "adamw")
    for step in range(3):
        for ps in (ours, theirs, plain):
            for p, g in zip(ps, _grads_for(ps, step, rel_norm)):
                p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        o.step(); t.step(); u.step()
        assert abs(float(o.grad_norm) - rel_norm) < 1e-5
        assert float(o.clip_state[1]) == (1.0 if rel_norm < 1 else
                                          pytest.approx(0.5, abs=1e-5))
        for a, b in zip(ours, theirs):
            assert torch.allclose(a, b, rtol=0, atol=1e-6)
        if rel_norm < 1:               # coef == 1: the unclipped bits
            for a, b in zip(ours, plain):
                assert torch.equal(a.detach().view(torch.int32),
                                   b.detach().view(torch.int32))
    assert o.skipped_steps() == 0


def test_zero_grads_are_pure_decay():
    for kind in ("sgd", "adam"):
        ps = _two_tensor_model()
        p0 = [p.detach().clone() for p in ps]
        o = (FusedSGD(ps, lr=0.1, weight_decay=0.5, max_grad_norm=1.0)
             if kind == "sgd" else
             FusedAdam(ps, lr=0.1, weight_decay=0.5, max_grad_norm=1.0,
                       decoupled_weight_decay=True))
        for p in ps:
            p.grad = torch.zeros_like(p)
        o.step()
        assert float(o.grad_norm) == 0.0
        assert o.clip_state.tolist() == [0.0, 1.0, 1.0, 0.0]
        for p, q in zip(ps, p0):
            assert torch.isfinite(p).all()
            assert torch.allclose(p, q * (1 - 0.1 * 0.5), rtol=0, atol=1e-6)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_fallback_skips_a_non_finite_step(kind, bad):
    ps = _two_tensor_model()
    o = _make(kind, ps, 1.0)
    for p, g in zip(ps, _grads_for(ps, 0, 2.0)):
        p.grad = g
    o.step()                                          # state becomes non-zero
    state = o.momentum_bufs if kind == "sgd" else o.exp_avg + o.exp_avg_sq
    before = [t.detach().clone() for t in list(ps) + state]
    for p, g in zip(ps, _grads_for(ps, 1, 2.0)):
        p.grad = g
    ps[1].grad[3] = bad
    o.step()
    assert o.skipped_steps() == 1
    assert o.clip_state[1] == 0.0 and o.clip_state[2] == 0.0
    for a, b in zip(list(ps) + state, before):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
    for p, g in zip(ps, _grads_for(ps, 2, 2.0)):
        p.grad = g
    o.step()                                          # the next step trains
    assert o.skipped_steps() == 1 and o.clip_state[2] == 1.0
    for a, b in zip(ps, before):
        assert torch.isfinite(a).all() and not torch.equal(a.detach(), b)


def _mixed_model():
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.BatchNorm1d(16),
                      nn.Linear(16, 4))
    m[0] = m[0].to(torch.bfloat16)
    m[3] = m[3].to(torch.bfloat16)
    return m


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_arena_norm_spans_the_dtype_groups(kind):
    m1, m2 = _mixed_model(), _mixed_model()
    arena = FlatParamArena(m1)
    assert {g.dtype for g in arena.groups} == {torch.float32, torch.bfloat16}
    kw = dict(lr=0.05, weight_decay=0.01, max_grad_norm=1.0)
    cls = FusedSGD if kind == "sgd" else FusedAdam
    o1, o2 = cls.from_arena(arena, **kw), cls(m2.parameters(), **kw)
    for step in range(3):
        gen = torch.Generator().manual_seed(step)
        gs = [torch.randn(p.shape, generator=gen).to(p.dtype)
              for p in m2.parameters()]
        for p1, p2, g in zip(m1.parameters(), m2.parameters(), gs):
            p1.grad.copy_(g)
            p2.grad = g.clone()
        o1.step(); o2.step()
        ref = ref_norm(*gs)
        assert ref > 2.0                               # clipped
        for o in (o1, o2):
            assert abs(float(o.grad_norm) / ref - 1) < 1e-6
        for p1, p2 in zip(m1.parameters(), m2.parameters()):
            # The two sum the squares in different orders, so coef may differ
            # by an fp32 ulp. The fp32 group shows the shared norm sharply (a
            # norm per group would move it by lr / 10). The fallback rounds a
            # bf16 update (at most 4 lr here) and the bf16 sum, where that ulp
            # can flip one bf16 ulp (2^-7) of each, in every step so far.
            if p1.dtype == torch.float32:
                assert torch.allclose(p1, p2, rtol=0, atol=1e-6)
            else:
                tol = (step + 1) * 2.0 ** -7 * (4 * 0.05 + p2.float().abs())
                assert ((p1.float() - p2.float()).abs() <= tol).all()


def test_config_round_trip():
    cfg = BatonConfig.from_dict(
        {"train": {"optimizer": "adamw", "max_grad_norm": 1.0,
                   "weight_decay": 0.01}})
    assert cfg.train.max_grad_norm == 1.0 and cfg.train.optimizer == "adamw"
    again = BatonConfig.from_dict(
        {k: v for k, v in cfg.to_dict().items() if v is not None})
    assert again.train == cfg.train
    o = make_optimizer(_two_tensor_model(), cfg.train)
    assert isinstance(o, FusedAdam) and o.decoupled_weight_decay
    assert o.max_grad_norm == 1.0 and o.clip_state is not None
    d = TrainConfig()
    assert d.max_grad_norm == 0.0
    o = make_optimizer(_two_tensor_model(), d)
    assert isinstance(o, FusedSGD) and o.max_grad_norm is None
    assert o.clip_state is None and o.grad_norm is None
    assert not o.decoupled_weight_decay and o.skipped_steps() == 0
    o = make_optimizer(_two_tensor_model(),
                       TrainConfig(optimizer="adam", max_grad_norm=math.inf))
    assert not o.decoupled_weight_decay and o.max_grad_norm == math.inf
    with pytest.raises(ValueError, match="unknown optimizer"):
        make_optimizer(_two_tensor_model(), TrainConfig(optimizer="lion"))
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedSGD(_two_tensor_model(), max_grad_norm=-1.0)


# ---- GPU ---------------------------------------------------------------------

DTYPES = [torch.float32, torch.bfloat16]
DEV = "cuda:0"


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def measure(ops, gs, max_norm, state=None):
    """grad_sumsq per tensor at consecutive offsets, then clip_finalize."""
    total = sum(grid_of(g.numel()) for g in gs)
    partials = torch.full((total,), math.nan, device=DEV)
    state = torch.zeros(4, device=DEV) if state is None else state
    off = 0
    for g in gs:
        nb = ops.grad_sumsq(g, partials, off)
        assert nb == grid_of(g.numel()) == ops.optim_grid(g.numel())
        off += nb
    ops.clip_finalize(partials, off, max_norm, state)
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", range(7))
def test_norm_against_float64(dtype, which):
    ops = require_hip()
    V = VEC[dtype]
    n = norm_sizes(V)[which]
    x = make_input(n, dtype)
    g = x.to(DEV)
    st = measure(ops, [g], math.inf).cpu()
    again = measure(ops, [g], math.inf).cpu()
    ref = ref_norm(x)
    ratio = abs(float(st[0]) / ref - 1.0) / norm_bound(chain_of(n, V))
    print(f"norm {dtype} n={n}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert same_bits(st, again)
    assert st.tolist()[1:] == [1.0, 1.0, 0.0]


@pytest.mark.gpu
def test_two_groups_one_norm():
    ops = require_hip()
    xs = [make_input(10007, torch.bfloat16), make_input(1025, torch.float32)]
    st = measure(ops, [x.to(DEV) for x in xs], math.inf).cpu()
    ref = ref_norm(*xs)
    assert max(ref_norm(x) for x in xs) < 0.95 * ref    # either group shows
    T = max(chain_of(10007, 8), chain_of(1025, 4))
    assert abs(float(st[0]) / ref - 1.0) <= norm_bound(T)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_coef(dtype):
    ops = require_hip()
    x = make_input(10007, dtype)
    g = x.to(DEV)
    nrm = ref_norm(x)
    st = measure(ops, [g], 2.0 * nrm).cpu()
    assert st.tolist()[1:] == [1.0, 1.0, 0.0]
    st = measure(ops, [g], 0.5 * nrm).cpu()
    ref = ref_coef(st[0], 0.5 * nrm)
    ratio = abs(float(st[1]) / ref - 1.0) / COEF_BOUND
    print(f"coef {dtype}: {ratio:.3f} of the bound")
    assert 0.4 < ref < 0.6 and ratio <= 1.0
    st = measure(ops, [g], math.inf).cpu()
    assert st[1] == 1.0
    st = measure(ops, [torch.zeros_like(g)], 1.0).cpu()
    assert st.tolist() == [0.0, 1.0, 1.0, 0.0]


SGD_HP = dict(lr=0.1, momentum=0.9, weight_decay=0.1)
ADAM_HP = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1,
               bc1=1 - 0.9 ** 3, bc2=1 - 0.999 ** 3)
N_STEP = 10007


def step_inputs(dtype, g_cpu=None, n=N_STEP):
    p0, g, m0, v0 = _step_case(dtype, n)
    t = lambda a, dt: torch.from_numpy(a).to(dt).to(DEV)
    g = t(g, dtype) if g_cpu is None else g_cpu.to(DEV)
    return t(p0, dtype), g, t(m0, torch.float32), t(v0, torch.float32)


def run_step(ops, opt, tensors, zero, ext, state=None, decoupled=False):
    p, g, m, v = (x.clone() for x in tensors)
    if opt == "sgd":
        args = (p, g, m, SGD_HP["lr"], SGD_HP["momentum"],
                SGD_HP["weight_decay"], zero)
        ops.sgd_step_ext(*args, state, decoupled) if ext else ops.sgd_step(*args)
    else:
        h = ADAM_HP
        args = (p, g, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"],
                h["weight_decay"], h["bc1"], h["bc2"], zero)
        ops.adam_step_ext(*args, state, decoupled) if ext else ops.adam_step(*args)
    return p, g, m, v


def check_ext_step_with_coef_one(ops, dtype, opt, zero, n):
    tensors = step_inputs(dtype, n=n)
    st = measure(ops, [tensors[1]], math.inf)
    assert st[1].item() == 1.0
    dense = run_step(ops, opt, tensors, zero, ext=False)
    for state in (st, None):
        out = run_step(ops, opt, tensors, zero, ext=True, state=state)
        for a, b in zip(out, dense):
            assert same_bits(a, b)
    assert (dense[1] == 0).all() if zero else same_bits(dense[1], tensors[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("zero", [False, True], ids=["keep_g", "zero_g"])
def test_ext_step_with_coef_one_is_the_dense_step(dtype, opt, zero):
    check_ext_step_with_coef_one(require_hip(), dtype, opt, zero, N_STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", range(7))
def test_ext_step_with_coef_one_flat_sizes(dtype, which):
    ops = require_hip()
    n = step_sizes(VEC[dtype])[which]
    for opt in ("sgd", "adam"):
        for zero in (False, True):
            check_ext_step_with_coef_one(ops, dtype, opt, zero, n)


def check_fp32_clipped_step(ops, opt, n):
    tensors = step_inputs(torch.float32, n=n)
    st = measure(ops, [tensors[1]], 0.5 * ref_norm(tensors[1].cpu()))
    assert 0.4 < st[1].item() < 0.6
    out = run_step(ops, opt, tensors, False, ext=True, state=st)
    scaled = (tensors[0], tensors[1] * st[1], tensors[2], tensors[3])
    dense = run_step(ops, opt, scaled, False, ext=False)
    for a, b in zip((out[0], out[2], out[3]), (dense[0], dense[2], dense[3])):
        assert same_bits(a, b)
    assert same_bits(out[1], tensors[1])


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_fp32_clipped_step_is_the_dense_step_on_coef_g(opt):
    check_fp32_clipped_step(require_hip(), opt, N_STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(7))
def test_fp32_clipped_step_flat_sizes(which):
    ops = require_hip()
    for opt in ("sgd", "adam"):
        check_fp32_clipped_step(ops, opt, step_sizes(4)[which])


def check_bf16_clipped_step(ops, opt, n):
    tensors = step_inputs(torch.bfloat16, n=n)
    st = measure(ops, [tensors[1]], 0.5 * ref_norm(tensors[1].cpu()))
    coef = st[1].item()
    assert 0.4 < coef < 0.6
    out = run_step(ops, opt, tensors, False, ext=True, state=st)
    p0, g, m0, v0 = (x.float().cpu().numpy() for x in tensors)
    p = out[0].float().cpu().numpy()
    if opt == "sgd":
        r = sgd_ratio(p, p0, g, m0, SGD_HP["lr"], SGD_HP["momentum"],
                      SGD_HP["weight_decay"], coef, 2.0 ** -8)
    else:
        h = ADAM_HP
        r = adam_ratio(p, p0, g, m0, v0, h["lr"], h["beta1"], h["beta2"],
                       h["eps"], h["weight_decay"], h["bc1"], h["bc2"], coef,
                       2.0 ** -8, decoupled=False)
    print(f"bf16 clipped {opt} n={n}: p {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_bf16_clipped_step_against_float64(opt):
    check_bf16_clipped_step(require_hip(), opt, N_STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(7))
def test_bf16_clipped_step_flat_sizes(which):
    ops = require_hip()
    for opt in ("sgd", "adam"):
        check_bf16_clipped_step(ops, opt, step_sizes(8)[which])


def check_fp32_decoupled_step(ops, opt, clip, n):
    tensors = step_inputs(torch.float32, n=n)
    st, coef = None, 1.0
    if clip:
        st = measure(ops, [tensors[1]], 0.5 * ref_norm(tensors[1].cpu()))
        coef = st[1].item()
    out = run_step(ops, opt, tensors, False, ext=True, state=st, decoupled=True)
    p0, g, m0, v0 = (x.cpu().numpy() for x in tensors)
    p = out[0].cpu().numpy()
    u = 2.0 ** -23
    if opt == "sgd":
        # p' = p0 (1 - lr wd), then the chain of the SGD bound without wd
        lr, mu, wd = (float(np.float32(SGD_HP[k]))
                      for k in ("lr", "momentum", "weight_decay"))
        p064, g64, m64 = (np.asarray(a, np.float64) for a in (p0, g, m0))
        ref = p064 * (1 - lr * wd) - lr * (mu * m64 + coef * g64)
        bound = u * np.abs(ref) + 3 * E * lr * (np.abs(coef * g64)
                                                + wd * np.abs(p064)
                                                + mu * np.abs(m64))
        r = float(np.max(np.abs(p - ref) / bound))
    else:
        h = ADAM_HP
        r = adam_ratio(p, p0, g, m0, v0, h["lr"], h["beta1"], h["beta2"],
                       h["eps"], h["weight_decay"], h["bc1"], h["bc2"], coef, u,
                       decoupled=True)
    print(f"fp32 decoupled {opt} clip={clip} n={n}: p {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_fp32_decoupled_step_against_float64(opt, clip):
    check_fp32_decoupled_step(require_hip(), opt, clip, N_STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(7))
def test_fp32_decoupled_step_flat_sizes(which):
    ops = require_hip()
    for opt in ("sgd", "adam"):
        for clip in (False, True):
            check_fp32_decoupled_step(ops, opt, clip, step_sizes(4)[which])


def check_non_finite_step_is_skipped(ops, dtype, bad, zero, n):
    x = make_input(n, dtype).clone()
    if bad == "inf_last_tail":
        x[-1] = math.inf
    else:
        x[min(1, n - 1)] = math.nan
    tensors = step_inputs(dtype, x, n=n)
    good = step_inputs(dtype, n=n)
    for opt in ("sgd", "adam"):
        st = torch.tensor([0.0, 1.0, 1.0, 2.0], device=DEV)
        measure(ops, [tensors[1]], 1.0, st)
        assert st.tolist()[1:] == [0.0, 0.0, 3.0]
        p, g, m, v = run_step(ops, opt, tensors, zero, ext=True, state=st)
        assert same_bits(p, tensors[0])
        assert same_bits(m, tensors[2]) and same_bits(v, tensors[3])
        if zero:
            assert torch.equal(bits(g), torch.zeros_like(bits(g)))  # all +0.0
        else:
            assert same_bits(g, tensors[1])
        # the following finite step is the dense step
        measure(ops, [good[1]], math.inf, st)
        assert st.tolist()[1:] == [1.0, 1.0, 3.0]
        after = (p, good[1], m, v)
        for a, b in zip(run_step(ops, opt, after, zero, ext=True, state=st),
                        run_step(ops, opt, after, zero, ext=False)):
            assert same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("bad", ["inf_last_tail", "nan_first_vector"])
@pytest.mark.parametrize("zero", [False, True], ids=["keep_g", "zero_g"])
def test_non_finite_step_is_skipped(dtype, bad, zero):
    assert N_STEP % VEC[dtype]                      # there is a tail
    check_non_finite_step_is_skipped(require_hip(), dtype, bad, zero, N_STEP)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", range(7))
def test_non_finite_step_is_skipped_flat_sizes(dtype, which):
    ops = require_hip()
    n = step_sizes(VEC[dtype])[which]
    for bad in ("inf_last_tail", "nan_first_vector"):
        for zero in (False, True):
            check_non_finite_step_is_skipped(ops, dtype, bad, zero, n)


@pytest.mark.gpu
def test_graph_replay_equals_eager():
    def build():
        torch.manual_seed(5)
        m = nn.Sequential(nn.Linear(8, 16), nn.Linear(16, 4, bias=False)).to(DEV)
        arena = FlatParamArena(m)
        return arena, FusedSGD.from_arena(arena, lr=0.1, momentum=0.9,
                                          max_grad_norm=1.0)

    (a_e, o_e), (a_g, o_g) = build(), build()
    n = a_e.groups[0].flat.numel()
    assert len(list(a_e.model.parameters())) == 3 and n == 208
    gen = torch.Generator().manual_seed(9)
    unit = torch.randn(n, generator=gen)
    unit = unit / unit.norm()
    bad = unit.clone()
    bad[n - 1] = math.inf
    warm = (0.3 * unit).to(DEV)
    for a, o in ((a_e, o_e), (a_g, o_g)):            # momentum becomes non-zero
        a.groups[0].grad.copy_(warm)
        o.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g.step()
    expect = [(1.0, 1.0, 0.0), (None, 1.0, 0.0), (0.0, 0.0, 1.0)]
    for fill, exp in zip((0.5 * unit, 2.0 * unit, bad), expect):
        fill = fill.to(DEV)
        a_e.groups[0].grad.copy_(fill)
        a_g.groups[0].grad.copy_(fill)
        o_e.step()
        graph.replay()
        torch.cuda.synchronize()
        st = o_g.clip_state.tolist()
        assert tuple(st[1:]) == exp or (exp[0] is None and 0.4 < st[1] < 0.6
                                        and tuple(st[2:]) == exp[1:])
        assert same_bits(o_g.clip_state, o_e.clip_state)
        assert same_bits(a_g.groups[0].flat, a_e.groups[0].flat)
        assert same_bits(o_g.momentum_bufs[0], o_e.momentum_bufs[0])
        assert (a_g.groups[0].grad == 0).all()        # zero_grad stays fused
    assert o_g.skipped_steps() == 1


@pytest.mark.gpu
def test_refusals():
    ops = require_hip()
    f = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    g, partials, state = f(64), f(8), f(4)

    def refused(match, fn, *a):
        with pytest.raises(RuntimeError, match=match):
            fn(*a)

    # g / p / m / v: contiguous, 16-byte aligned, on one device
    refused("g must be contiguous", ops.grad_sumsq, f(128)[::2], partials, 0)
    refused("g must be 16-byte aligned", ops.grad_sumsq, f(65)[1:], partials, 0)
    refused("g must be on the GPU", ops.grad_sumsq, g.cpu(), partials, 0)
    sgd = lambda p, g_, m, st=None: ops.sgd_step_ext(
        p, g_, m, 0.1, 0.9, 0.0, False, st, False)
    adam = lambda p, g_, m, v, st=None: ops.adam_step_ext(
        p, g_, m, v, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, False, st, False)
    refused("p must be contiguous", sgd, f(128)[::2], g, f(64))
    refused("p must be 16-byte aligned", sgd, f(65)[1:], g, f(64))
    refused("g must be on the GPU", sgd, f(64), g.cpu(), f(64))
    refused("m must be 16-byte aligned", sgd, f(64), g, f(65)[1:])
    refused("m must be contiguous", adam, f(64), g, f(128)[::2], f(64))
    refused("v must be 16-byte aligned", adam, f(64), g, f(64), f(65)[1:])
    refused("v must be on the GPU", adam, f(64), g, f(64), f(64).cpu())
    refused("g must have p's dtype", sgd, f(64, torch.bfloat16), g, f(64))
    # partials / clip_state: contiguous fp32 on that device
    refused("partials must be fp32", ops.grad_sumsq, g,
            f(8, torch.bfloat16), 0)
    refused("partials must be contiguous", ops.grad_sumsq, g, f(16)[::2], 0)
    refused("partials must be on the gradients' device", ops.grad_sumsq, g,
            partials.cpu(), 0)
    refused("clip_state must be fp32", ops.clip_finalize, partials, 1, 1.0,
            f(4, torch.bfloat16))
    refused("clip_state must be contiguous", ops.clip_finalize, partials, 1,
            1.0, f(8)[::2])
    refused("clip_state must be on the gradients' device", sgd, f(64), g,
            f(64), state.cpu())
    # clip_state has 4 elements
    refused("clip_state must have 4 elements", ops.clip_finalize, partials, 1,
            1.0, f(3))
    refused("clip_state must have 4 elements", adam, f(64), g, f(64), f(64),
            f(5))
    # offset + nblocks, count within partials
    refused("beyond partials", ops.grad_sumsq, g, partials, 8)
    refused("beyond partials", ops.grad_sumsq, g, partials, -1)
    refused("beyond partials", ops.clip_finalize, partials, 9, 1.0, state)
    # max_norm
    for bad in (math.nan, 0.0, -1.0):
        refused("max_norm must be > 0", ops.clip_finalize, partials, 1, bad,
                state)
    torch.cuda.synchronize()
    assert state.tolist() == [0.0, 0.0, 0.0, 0.0]     # nothing was launched

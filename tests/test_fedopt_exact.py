"""The federated server step (ops/csrc/fedopt.hip: delta_sumsq_kernel,
delta_scale_cast_kernel, fedopt_finalize_kernel, server_step_kernel) against
float64 from the stored inputs, and ``fedopt_arena`` on RCCL at world 1.

Notation: e = 2^-24, one fp32 rounding. The threshold is 1.0 of each bound
below; nothing is fitted.

The norm. delta_sumsq_kernel is grad_sumsq_kernel on d = fl(float(theta) - x):
the bound of tests/test_optim_clip.py for the chain of T fmas, the shuffles,
the wave sums, the square root and the store, plus the one rounding of the
subtraction (relative to the exact difference, so e on the norm as well):

    |norm / ref - 1| <= (T + 12) 2^-25 + 2^-23 + e
    |coef / ref - 1| <= 2^-22     (against the coefficient recomputed in
                                   float64 from the STORED fp32 norm)

The cast. dst = fl(fl(alpha coef) fl(float(theta) - x)): a multiply, a
subtract and a multiply, none of which can contract to an fma, so the check is
for bits against the same three torch fp32 operations on the device.

The step. inv_W and every scalar are the fp32 values the kernel holds; the
reference is float64 from the stored D, x0, m0, v0. K = 1 + 2^-10 covers the
second-order terms, rD is the relative error of Delta^ = fl(D inv_W): e.

    mean        x = fl(x0 + Delta^)
                |x - ref| <= K (rD |Delta| + e |ref|)
    fedavgm     m = fma(b1, m0, Delta^):       dm = rD |Delta| + e |m|
                x = fma(lr, m, x0):            dx = lr dm + e |x|
    adaptive    m = fma(b1, m0, fl(fl(1 - b1) Delta^)): the difference, the
                product and Delta^ itself, then the fma:
                                               dm = (rD + 2 e)(1 - b1)|Delta| + e |m|
      fedadagrad  v = fma(Delta^, Delta^, v0): dv = 2 rD Delta^2 + e v
      fedadam     v = fma(b2, v0, fl(fl(fl(1 - b2) Delta^) Delta^)): the
                  difference, two products, Delta^ twice, then the fma:
                                               dv = (2 rD + 3 e)(1 - b2) Delta^2 + e v
      fedyogi     d2 = fl(Delta^ Delta^) (2 rD + e), u = fl(fl(fl(1 - b2) d2)
                  sign) (the difference and one product; the sign is exact),
                  v = fl(v0 - u):              dv = (2 rD + 3 e)(1 - b2) Delta^2 + e v
                  where |v0 - Delta^2| <= (2 rD + 2 e) Delta^2 the kernel's
                  sign(v0 - d2) may be any of -1, 0, 1 while the reference's is
                  fixed: there dv grows by 2 (1 - b2) Delta^2. (The planted
                  equalities v0 == d2 are checked for bits as well: v keeps
                  v0's bits.)
                x = fma(lr, fl(m / fl(fl(sqrt(v)) + tau)), x0): sqrt and
                division taken as correctly rounded. The square root halves
                dv / v and rounds (e), the sum rounds (e):
                                               rd = dv / (2 v) + 2 e
                the quotient rounds once more: dq = (dm + |m| (rd + e)) / denom
                                               dx = lr dq + e |x|
    every bound is multiplied by K.

Inputs cover Delta = 0, v0 = tau^2, |Delta| from 2^-20 to 2^10, and Yogi with
v0 above, below and equal to d2.

The world-1 RCCL test holds ``fedopt_arena`` against ``ServerOptimizer`` on the
CPU round by round from the device's stored state: both evaluate the same
definition, D from the same fl(theta - x) with coefficients that each meet the
norm and coef bounds above, so the float64 step from the oracle's D bounds the
device with rD = e + 2 (e + 2^-22 + (T + 12) 2^-25 + 2^-23 + e).

The unmarked tests emulate the index walk, the capped grid and the fp32
arithmetic in numpy: honest arithmetic meets every bound, and each single
defect exceeds 4x or fails an equality."""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

E = 2.0 ** -24
K2 = 1.0 + 2.0 ** -10
KBLOCK, KMAXGRID = 256, 2048
VEC = {torch.float32: 4, torch.bfloat16: 8}
DTYPES = [torch.float32, torch.bfloat16]
DEV = "cuda:0"
MODES = ["mean", "fedavgm", "fedadagrad", "fedadam", "fedyogi"]
HP = dict(lr=0.1, b1=0.9, b2=0.99, tau=1e-3)
PAD = 8                     # operands sit at element offset 8 of NaN parents
COEF_BOUND = 2.0 ** -22


def sizes(V):
    return [1, V - 1, V, V + 1, 255 * V + 3, 256 * V + 1, 4194333]


def grid_of(n):
    return min(KMAXGRID, max(1, -(-(n // 8 + 1) // KBLOCK)))


def chain_of(n, V):
    G = grid_of(n)
    return -(-(n // V) // (KBLOCK * G)) * V + (1 if n % V else 0)


def norm_bound(T):
    return (T + 12) * 2.0 ** -25 + 2.0 ** -23 + E


def f32(x):
    return np.asarray(x, dtype=np.float32)


def fma32(a, b, c):
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def bf16_round(x):
    u = f32(x).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def hp32():
    return {k: float(np.float32(v)) for k, v in HP.items()}


# ---- inputs (shared; never modified) ----------------------------------------

@functools.lru_cache(maxsize=None)
def make_pair(n, dtype):
    """(theta, x) on the CPU: x of unit variance, theta = x + d in dtype with
    d of scale 0.05 and |d| = 16 planted at the last element (the tail's, if
    there is one) and at the end of the last whole vector."""
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    d = 0.05 * torch.randn(n, generator=gen)
    V = VEC[dtype]
    d[n - 1] = 16.0
    if n >= V:
        d[(n // V) * V - 1] = -16.0
    return (x + d).to(dtype), x


def ref_delta_norm(theta, x):
    return math.sqrt(float((theta.double() - x.double()).pow(2).sum()))


def ref_coef(norm32, max_norm):
    return min(1.0, max_norm / (float(norm32) + 1e-6))


@functools.lru_cache(maxsize=None)
def step_inputs(n, inv_w):
    """D, x0, m0, v0 (numpy fp32) for one server step with that inv_W."""
    rng = np.random.default_rng(n)
    k = np.arange(n)
    tau2 = np.float32(np.float32(HP["tau"]) * np.float32(HP["tau"]))
    D = f32(rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n))
            * 2.0 ** ((k % 31) - 20.0))
    # |Delta| spans 2^-20 .. 2^10 whatever inv_W is
    D = f32(D / np.float32(inv_w))
    D[k % 7 == 3] = 0.0
    delta = D * np.float32(inv_w)
    d2 = delta * delta                                   # the kernel's fp32 d2
    v0 = f32(np.where(k % 2 == 0, 0.25, 4.0)) * d2        # Yogi: both signs
    v0[k % 11 == 5] = d2[k % 11 == 5]                     # and equality
    v0[(k % 5 == 1) | (D == 0.0)] = tau2
    x0 = f32(rng.standard_normal(n))
    m0 = f32(0.1 * rng.standard_normal(n))
    return D, x0, m0, f32(v0)


def yogi_equal(n, inv_w):
    D, _, _, v0 = step_inputs(n, inv_w)
    delta = D * np.float32(inv_w)
    return (v0 == delta * delta) & (D != 0.0)


# ---- float64 reference and bounds --------------------------------------------

def step_ref(mode, D, inv_w, x0, m0, v0, rD=E):
    """{name: (reference, bound)} of x, m, v after one applied step."""
    h = hp32()
    lr, b1, b2, tau = h["lr"], h["b1"], h["b2"], h["tau"]
    D, x0, m0, v0 = (np.asarray(a, np.float64) for a in (D, x0, m0, v0))
    delta = D * float(np.float32(inv_w))
    ad = np.abs(delta)
    if mode == "mean":
        x = x0 + delta
        return {"x": (x, K2 * (rD * ad + E * np.abs(x)))}
    if mode == "fedavgm":
        m = b1 * m0 + delta
        dm = rD * ad + E * np.abs(m)
        x = x0 + lr * m
        return {"x": (x, K2 * (lr * dm + E * np.abs(x))), "m": (m, K2 * dm)}
    m = b1 * m0 + (1 - b1) * delta
    dm = (rD + 2 * E) * (1 - b1) * ad + E * np.abs(m)
    d2 = delta * delta
    if mode == "fedadagrad":
        v = v0 + d2
        dv = 2 * rD * d2 + E * v
    elif mode == "fedadam":
        v = b2 * v0 + (1 - b2) * d2
        dv = (2 * rD + 3 * E) * (1 - b2) * d2 + E * v
    else:
        v = v0 - (1 - b2) * d2 * np.sign(v0 - d2)
        dv = (2 * rD + 3 * E) * (1 - b2) * d2 + E * np.abs(v)
        near = np.abs(v0 - d2) <= (2 * rD + 2 * E) * d2
        dv = dv + np.where(near, 2 * (1 - b2) * d2, 0.0)
    denom = np.sqrt(v) + tau
    rd = dv / (2 * v) + 2 * E
    dq = (dm + np.abs(m) * (rd + E)) / denom
    x = x0 + lr * m / denom
    return {"x": (x, K2 * (lr * dq + E * np.abs(x))), "m": (m, K2 * dm),
            "v": (v, K2 * dv)}


def worst_ratio(got, ref, bound):
    diff = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))   # a NaN fails


def step_ratios(mode, out, D, inv_w, x0, m0, v0, rD=E):
    ref = step_ref(mode, D, inv_w, x0, m0, v0, rD)
    return {k: worst_ratio(out[k], *ref[k]) for k in ref}


# ---- numpy emulation of the kernels ------------------------------------------

def covered(n, V, drop_tail=False, one_trip=False):
    """The elements the grid-stride walk of an n-element kernel touches."""
    nthr = grid_of(n) * KBLOCK
    nvec = n // V
    mask = np.zeros(n, bool)
    mask[: (min(nvec, nthr) if one_trip else nvec) * V] = True
    if not drop_tail:
        mask[nvec * V:] = True          # n % V < 256 threads: one trip
    return mask


def emu_delta_partials(theta, x, V, drop_tail=False, one_trip=False):
    """delta_sumsq_kernel: one fp32 partial per block."""
    d = f32(theta) - f32(x)
    n = d.size
    G = grid_of(n)
    nthr = G * KBLOCK
    nvec = n // V
    trips = max(1, -(-nvec // nthr))
    body = np.zeros(trips * nthr * V, np.float32)
    body[: nvec * V] = d[: nvec * V]
    body = body.reshape(trips, nthr, V)
    if one_trip:
        body = body[:1]
    body = body.transpose(1, 0, 2).reshape(nthr, -1)
    acc = np.zeros(nthr, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(body.shape[1]):
            acc = fma32(body[:, k], body[:, k], acc)
        if not drop_tail and n > nvec * V:
            tail = np.zeros(nthr, np.float32)
            tail[: n - nvec * V] = d[nvec * V:]
            acc = fma32(tail, tail, acc)
        v = acc.reshape(-1, 64)
        for off in (32, 16, 8, 4, 2, 1):
            w = v.copy()
            w[:, : 64 - off] = v[:, : 64 - off] + v[:, off:]
            v = w
        waves = v[:, 0].reshape(G, KBLOCK // 64)
        total = np.zeros(G, np.float32)
        for i in range(KBLOCK // 64):
            total = total + waves[:, i]
    return total


def emu_clip_finalize(partials, max_norm, skipped=0.0):
    """clip_finalize_kernel -> clip_state."""
    p = np.concatenate(partials).astype(np.float64)
    red = np.zeros(KBLOCK, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(min(KBLOCK, p.size)):
            red[t] = sum(p[t::KBLOCK], 0.0)         # in order
        w = KBLOCK // 2
        while w:
            red[:w] = red[:w] + red[w:2 * w]
            w //= 2
        sumsq = red[0]
        finite = bool(np.isfinite(sumsq))
        norm = np.sqrt(sumsq)
        c = min(1.0, max_norm / (norm + 1e-6))
    return f32([norm, c if finite else 0.0, 1.0 if finite else 0.0,
                skipped if finite else skipped + 1.0])


def emu_scale_cast(theta, x, alpha, state, V, ignore_coef=False,
                   read_theta_anyway=False, drop_tail=False, one_trip=False):
    """delta_scale_cast_kernel -> (dst over a NaN background, w_out)."""
    theta, x = f32(theta), f32(x)
    alpha = np.float32(alpha)
    finite = state[2] != 0.0
    w_out = alpha if finite else np.float32(0.0)
    dst = np.full(theta.size, np.nan, np.float32)
    mask = covered(theta.size, V, drop_tail, one_trip)
    with np.errstate(over="ignore", invalid="ignore"):
        if finite or read_theta_anyway:
            s = alpha if ignore_coef else alpha * state[1]
            dst[mask] = (s * (theta - x))[mask]
        else:
            dst[mask] = 0.0
    return dst, w_out


def emu_round_state(w_sum, skipped=0.0):
    """fedopt_finalize_kernel -> round_state."""
    W = np.float32(w_sum)
    applied = bool(np.isfinite(W) and W > 0)
    inv = np.float32(1.0 / np.float64(W)) if applied else np.float32(0.0)
    return f32([W, inv, 1.0 if applied else 0.0,
                skipped if applied else skipped + 1.0])


def emu_server_step(mode, D, x0, m0, v0, rs, drop_tail=False, one_trip=False,
                    no_omb1=False, no_sign=False, decay_adagrad=False,
                    skip_writes_m=False):
    """server_step_kernel<MODE> -> {x, m, v}."""
    h = {k: np.float32(v) for k, v in HP.items()}
    lr, b1, b2, tau = h["lr"], h["b1"], h["b2"], h["tau"]
    D, x, m, v = f32(D), f32(x0).copy(), f32(m0).copy(), f32(v0).copy()
    one = np.float32(1.0)
    if rs[2] == 0.0:
        if skip_writes_m:
            m = fma32(b1, m, D)
        return {"x": x, "m": m, "v": v}
    mask = covered(D.size, 4, drop_tail, one_trip)
    delta = D * rs[1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mode == "mean":
            xn, mn, vn = x + delta, m, v
        elif mode == "fedavgm":
            mn = fma32(b1, m, delta)
            xn, vn = fma32(lr, mn, x), v
        else:
            mn = fma32(b1, m, delta if no_omb1 else (one - b1) * delta)
            if mode == "fedadagrad":
                vn = (fma32(b2, v, delta * delta) if decay_adagrad
                      else fma32(delta, delta, v))
            elif mode == "fedadam":
                vn = fma32(b2, v, (one - b2) * delta * delta)
            else:
                d2 = delta * delta
                sign = one if no_sign else np.sign(v - d2)
                vn = v - (one - b2) * d2 * sign
            xn = fma32(lr, mn / (np.sqrt(vn) + tau), x)
    out = {}
    for name, new, old in (("x", xn, x), ("m", mn, m), ("v", vn, v)):
        out[name] = np.where(mask, f32(new), old)
    return out


def same_bits_np(a, b):
    return np.array_equal(f32(a).view(np.int32), f32(b).view(np.int32))


# ---- CPU: the emulation meets the bounds -------------------------------------

def _emu_norm(theta, x, V, max_norm, **mut):
    st = emu_clip_finalize(
        [emu_delta_partials(theta.float().numpy(), x.numpy(), V, **mut)],
        max_norm)
    ref = ref_delta_norm(theta, x)
    rn = abs(float(st[0]) / ref - 1.0) / norm_bound(chain_of(x.numel(), V))
    rc = abs(float(st[1]) / ref_coef(st[0], max_norm) - 1.0) / COEF_BOUND
    return rn, rc, st


def test_emulated_norm_and_cast_meet_the_bounds():
    for dtype in DTYPES:
        V = VEC[dtype]
        for n in sizes(V):
            theta, x = make_pair(n, dtype)
            nrm = ref_delta_norm(theta, x)
            for max_norm in (math.inf, 0.5 * nrm):
                rn, rc, st = _emu_norm(theta, x, V, max_norm)
                print(f"emu norm {dtype} n={n} clip={max_norm / nrm:.1f}: "
                      f"norm {rn:.3f} coef {rc:.3f}")
                assert rn <= 1.0 and rc <= 1.0
                assert st[2] == 1.0 and st[3] == 0.0
                if max_norm == math.inf:
                    assert st[1] == np.float32(1.0)
                else:
                    assert 0.4 < st[1] < 0.6
            if n > 300 * V:
                continue                   # the walk is covered() either way
            t, xx = theta.float().numpy(), x.numpy()
            dst, w = emu_scale_cast(t, xx, 0.25, st, V)
            want = (np.float32(0.25) * st[1]) * (t - xx)
            assert same_bits_np(dst, want) and w == np.float32(0.25)
    # the capped grid: a second trip plus a tail
    assert grid_of(4194333) == KMAXGRID
    assert 4194333 // 8 > KMAXGRID * KBLOCK and 4194333 % 8
    assert covered(4194333, 8).all() and covered(4194333, 4).all()


@pytest.mark.parametrize("mode", MODES)
def test_emulated_step_meets_the_bound(mode):
    for inv_w, w in ((1.0, 1.0), (float(np.float32(1.0 / 0.75)), 0.75)):
        rs = emu_round_state(w)
        assert rs[1] == np.float32(inv_w) and rs.tolist()[2:] == [1.0, 0.0]
        for n in sizes(4)[:-1] + [10007]:
            ins = step_inputs(n, inv_w)
            out = emu_server_step(mode, *ins, rs)
            r = step_ratios(mode, out, ins[0], inv_w, *ins[1:])
            print(f"emu {mode} n={n} inv_W={inv_w:.3f}: {r}")
            assert max(r.values()) <= 1.0
            if mode == "fedyogi":
                eq = yogi_equal(n, inv_w)
                assert same_bits_np(out["v"][eq], ins[3][eq])
    # W = 1, x0 = 0: Delta is D, bit for bit
    D = step_inputs(10007, 1.0)[0]
    z = np.zeros_like(D)
    out = emu_server_step("mean", D, z, z, z, emu_round_state(1.0))
    assert same_bits_np(out["x"], np.where(D == 0, 0.0, D))


def test_single_defects_exceed_4x_or_fail_an_equality():
    V, dtype = 8, torch.bfloat16
    # a skipped tail: the planted last element is the tail
    theta, x = make_pair(256 * V + 1, dtype)
    assert _emu_norm(theta, x, V, math.inf, drop_tail=True)[0] > 4.0
    # a second trip never taken: the planted end of the last whole vector
    theta, x = make_pair(4194333, dtype)
    assert _emu_norm(theta, x, V, math.inf, one_trip=True)[0] > 4.0
    assert _emu_norm(theta, x, V, math.inf)[0] <= 1.0
    # ... and in the elementwise kernels
    n = 256 * V + 1
    theta, x = make_pair(n, dtype)
    t, xx = theta.float().numpy(), x.numpy()
    nrm = ref_delta_norm(theta, x)
    st = emu_clip_finalize([emu_delta_partials(t, xx, V)], 0.5 * nrm)
    want = (np.float32(0.25) * st[1]) * (t - xx)
    assert not same_bits_np(emu_scale_cast(t, xx, 0.25, st, V,
                                           drop_tail=True)[0], want)
    assert not covered(4194333, V, one_trip=True).all()
    # coef ignored
    assert 0.4 < st[1] < 0.6
    assert not same_bits_np(emu_scale_cast(t, xx, 0.25, st, V,
                                           ignore_coef=True)[0], want)
    # theta read on a non-finite client
    tn = t.copy()
    tn[5] = np.nan
    bad = emu_clip_finalize([emu_delta_partials(tn, xx, V)], 1.0, skipped=2.0)
    assert bad.tolist()[1:] == [0.0, 0.0, 3.0]
    dst, w = emu_scale_cast(tn, xx, 0.25, bad, V)
    assert same_bits_np(dst, np.zeros(n)) and w == 0.0       # all +0.0
    dst, _ = emu_scale_cast(tn, xx, 0.25, bad, V, read_theta_anyway=True)
    assert not same_bits_np(dst, np.zeros(n))

    n = 10007
    inv_w = 2.0                                               # W = 0.5, N = 1
    ins = step_inputs(n, inv_w)
    rs = emu_round_state(0.5)
    ratios = lambda mode, out, inputs=ins: max(step_ratios(
        mode, out, inputs[0], inv_w, *inputs[1:]).values())
    assert ratios("fedadam", emu_server_step("fedadam", *ins, rs)) <= 1.0
    # a skipped tail / a second trip never taken in the step
    assert ratios("fedadam", emu_server_step("fedadam", *ins, rs,
                                             drop_tail=True)) > 4.0
    big = step_inputs(4194333, inv_w)
    out = emu_server_step("fedavgm", *big, rs, one_trip=True)
    assert ratios("fedavgm", out, big) > 4.0
    # division by N in place of W
    by_n = emu_round_state(0.5)
    by_n[1] = 1.0
    for mode in MODES:
        assert ratios(mode, emu_server_step(mode, *ins, by_n)) > 4.0
    # v started at 0 instead of tau^2 (the first round: m0 = 0)
    tau2 = np.float32(np.float32(HP["tau"]) ** 2)
    first = (ins[0], ins[1], np.zeros(n, np.float32),
             np.full(n, tau2, np.float32))
    for mode in ("fedadagrad", "fedadam", "fedyogi"):
        assert ratios(mode, emu_server_step(mode, *first, rs), first) <= 1.0
        out = emu_server_step(mode, first[0], first[1], first[2],
                              np.zeros(n, np.float32), rs)
        assert ratios(mode, out, first) > 4.0
    # Yogi's sign dropped
    assert ratios("fedyogi", emu_server_step("fedyogi", *ins, rs,
                                             no_sign=True)) > 4.0
    # adagrad's v decayed
    assert ratios("fedadagrad", emu_server_step("fedadagrad", *ins, rs,
                                                decay_adagrad=True)) > 4.0
    # m without the (1 - b1) factor
    for mode in ("fedadagrad", "fedadam", "fedyogi"):
        assert ratios(mode, emu_server_step(mode, *ins, rs,
                                            no_omb1=True)) > 4.0
    # a skipped round that still writes m: the check is for bits
    skip = emu_round_state(0.0, skipped=1.0)
    assert skip.tolist() == [0.0, 0.0, 0.0, 2.0]
    assert emu_round_state(np.nan).tolist()[1:] == [0.0, 0.0, 1.0]
    out = emu_server_step("fedadam", *ins, skip)
    assert all(same_bits_np(out[k], a) for k, a in zip("xmv", ins[1:]))
    out = emu_server_step("fedadam", *ins, skip, skip_writes_m=True)
    assert not same_bits_np(out["m"], ins[2])
    # x updated from the bf16 theta instead of the fp32 master
    out = emu_server_step("fedavgm", ins[0], bf16_round(ins[1]), ins[2],
                          ins[3], rs)
    assert ratios("fedavgm", out) > 4.0


# ---- GPU ---------------------------------------------------------------------

def native_ops():
    from baton_amd.ops._ext import hip_available, require_hip

    native_loaded = hip_available()
    assert native_loaded, "the in-tree HIP extension is not loaded"
    return require_hip()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def in_parent(t, dtype=None):
    """t at element offset PAD of a NaN-filled device parent: (parent, view)."""
    t = torch.as_tensor(t)
    dtype = dtype or t.dtype
    parent = torch.full((t.numel() + 2 * PAD,), math.nan, dtype=dtype,
                        device=DEV)
    view = parent[PAD: PAD + t.numel()]
    view.copy_(t.to(dtype))
    return parent, view


def canaries_alive(parent):
    return bool(torch.isnan(parent[:PAD]).all()
                and torch.isnan(parent[-PAD:]).all())


def measure(ops, theta, x, max_norm, state=None):
    n = theta.numel()
    partials = torch.full((grid_of(n) + 3,), math.nan, device=DEV)
    state = torch.zeros(4, device=DEV) if state is None else state
    nb = ops.delta_sumsq(theta, x, partials, 3)
    assert nb == grid_of(n) == ops.optim_grid(n)
    assert torch.isnan(partials[:3]).all()
    ops.clip_finalize(partials[3:], nb, max_norm, state)
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", range(7))
def test_delta_norm_and_cast(dtype, which):
    ops = native_ops()
    V = VEC[dtype]
    n = sizes(V)[which]
    theta_c, x_c = make_pair(n, dtype)
    (tp, theta), (xp, x) = in_parent(theta_c), in_parent(x_c)
    ref = ref_delta_norm(theta_c, x_c)
    st = measure(ops, theta, x, math.inf).cpu()
    again = measure(ops, theta, x, math.inf).cpu()
    ratio = abs(float(st[0]) / ref - 1.0) / norm_bound(chain_of(n, V))
    print(f"delta norm {dtype} n={n}: {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert same_bits(st, again)
    assert st.tolist()[1:] == [1.0, 1.0, 0.0]
    state = measure(ops, theta, x, 0.5 * ref)
    coef = state.cpu()
    rc = abs(float(coef[1]) / ref_coef(coef[0], 0.5 * ref) - 1.0) / COEF_BOUND
    print(f"coef {dtype} n={n}: {rc:.3f} of the bound")
    assert 0.4 < float(coef[1]) < 0.6 and rc <= 1.0

    # the cast: three fp32 operations, for bits
    alpha = 0.3
    dp, dst = in_parent(torch.zeros(n))
    w_out = torch.full((1,), math.nan, device=DEV)
    ops.delta_scale_cast(dst, theta, x, alpha, state, w_out)
    alpha_t = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    want = (alpha_t * state[1]) * (theta.float() - x)
    assert same_bits(dst, want)
    assert w_out.item() == alpha_t.item()
    # a non-finite client: +0.0 everywhere, NaN in theta never read
    theta[n // 2] = math.nan
    bad = measure(ops, theta, x, 1.0, torch.tensor([0., 1., 1., 2.],
                                                   device=DEV))
    assert bad.tolist()[1:] == [0.0, 0.0, 3.0]
    dst.fill_(math.nan)
    ops.delta_scale_cast(dst, theta, x, alpha, bad, w_out)
    assert torch.equal(bits(dst), torch.zeros_like(bits(dst)))
    assert w_out.item() == 0.0
    dst.fill_(math.nan)
    ops.delta_scale_cast(dst, theta, x, alpha, bad)  # w_out may be left out
    assert torch.equal(bits(dst), torch.zeros_like(bits(dst)))
    for parent in (tp, xp, dp):
        assert canaries_alive(parent)
    assert same_bits(x, x_c.to(DEV))


def gpu_round_state(ops, w, state=None):
    state = torch.zeros(4, device=DEV) if state is None else state
    ops.fedopt_finalize(torch.tensor([w], dtype=torch.float32, device=DEV),
                        state)
    return state


def gpu_step(ops, mode, ins, rs):
    D, x0, m0, v0 = ins
    parents = [in_parent(a) for a in (D, x0, m0, v0)]
    (_, Dv), (_, xv), (_, mv), (_, vv) = parents
    h = HP
    ops.server_step(mode, Dv, xv, mv if mode != "mean" else None,
                    vv if mode in MODES[2:] else None, h["lr"], h["b1"],
                    h["b2"], h["tau"], rs)
    for p, _ in parents:
        assert canaries_alive(p)
    assert same_bits(Dv, torch.from_numpy(D).to(DEV))
    return {"x": xv.cpu().numpy(), "m": mv.cpu().numpy(),
            "v": vv.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", range(7))
def test_server_step_against_float64(mode, which):
    ops = native_ops()
    n = sizes(4)[which]
    inv_w = float(np.float32(1.0 / 0.75))
    rs = gpu_round_state(ops, 0.75)
    assert rs.tolist() == [0.75, inv_w, 1.0, 0.0]
    ins = step_inputs(n, inv_w)
    out = gpu_step(ops, mode, ins, rs)
    r = step_ratios(mode, out, ins[0], inv_w, *ins[1:])
    print(f"{mode} n={n}: {r} of the bounds")
    assert max(r.values()) <= 1.0
    # what the mode does not own keeps its bits
    if mode in ("mean", "fedavgm"):
        assert same_bits_np(out["v"], ins[3])
    if mode == "mean":
        assert same_bits_np(out["m"], ins[2])
    if mode == "fedyogi":
        eq = yogi_equal(n, inv_w)
        assert same_bits_np(out["v"][eq], ins[3][eq])


@pytest.mark.gpu
def test_delta_is_d_with_unit_weight():
    ops = native_ops()
    n = 10007
    rs = gpu_round_state(ops, 1.0)
    assert rs.tolist() == [1.0, 1.0, 1.0, 0.0]
    D = step_inputs(n, 1.0)[0]
    z = np.zeros_like(D)
    out = gpu_step(ops, "mean", (D, z, z, z), rs)
    assert same_bits_np(out["x"], np.where(D == 0, 0.0, D))
    # fedyogi with inv_W = 1: both signs and the planted equalities
    ins = step_inputs(n, 1.0)
    out = gpu_step(ops, "fedyogi", ins, rs)
    assert max(step_ratios("fedyogi", out, ins[0], 1.0, *ins[1:]).values()) <= 1
    eq = yogi_equal(n, 1.0)
    assert eq.sum() > 100 and same_bits_np(out["v"][eq], ins[3][eq])
    d2 = np.float64(ins[0]) ** 2
    assert ((ins[3] > d2).sum() > 100) and ((ins[3] < d2).sum() > 100)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [0.0, math.nan, math.inf, -1.0])
def test_skipped_round_keeps_every_bit(w):
    ops = native_ops()
    n = 256 * 4 + 1
    ins = step_inputs(n, 1.0)
    rs = gpu_round_state(ops, w)
    assert rs.tolist()[1:] == [0.0, 0.0, 1.0]
    for mode in MODES:
        out = gpu_step(ops, mode, ins, rs)
        for k, a in zip("xmv", ins[1:]):
            assert same_bits_np(out[k], a)
    gpu_round_state(ops, w, rs)
    assert rs.tolist()[1:] == [0.0, 0.0, 2.0]
    gpu_round_state(ops, 0.5, rs)                    # an applied round
    assert rs.tolist() == [0.5, 2.0, 1.0, 2.0]


@pytest.mark.gpu
def test_refusals():
    ops = native_ops()
    f = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    bf = torch.bfloat16
    theta, x, partials, state = f(64, bf), f(64), f(8), f(4)

    def refused(match, fn, *a):
        with pytest.raises(RuntimeError, match=match):
            fn(*a)

    # delta_sumsq
    ds = ops.delta_sumsq
    refused("theta must be contiguous", ds, f(128, bf)[::2], x, partials, 0)
    refused("theta must be 16-byte aligned", ds, f(65, bf)[1:], x, partials, 0)
    refused("theta must be on the GPU", ds, theta.cpu(), x, partials, 0)
    refused("theta must be fp32 or bf16", ds, f(64, torch.float16), x,
            partials, 0)
    refused("x must be fp32", ds, theta, f(64, bf), partials, 0)
    refused("x must have 64 elements", ds, theta, f(68), partials, 0)
    refused("x must be 16-byte aligned", ds, theta, f(65)[1:], partials, 0)
    refused("x must be on the GPU", ds, theta, x.cpu(), partials, 0)
    refused("partials must be fp32", ds, theta, x, f(8, bf), 0)
    refused("partials must be contiguous", ds, theta, x, f(16)[::2], 0)
    refused("beyond partials", ds, theta, x, partials, 8)
    refused("beyond partials", ds, theta, x, partials, -1)
    # delta_scale_cast
    dc = ops.delta_scale_cast
    dst = f(64)
    refused("dst must be fp32", dc, f(64, bf), theta, x, 0.5, state, None)
    refused("dst must have 64 elements", dc, f(60), theta, x, 0.5, state, None)
    refused("dst must be contiguous", dc, f(128)[::2], theta, x, 0.5, state,
            None)
    refused("x must be contiguous", dc, dst, theta, f(128)[::2], 0.5, state,
            None)
    refused("theta must be 16-byte aligned", dc, dst, f(65, bf)[1:], x, 0.5,
            state, None)
    refused("clip_state must have 4 elements", dc, dst, theta, x, 0.5, f(8),
            None)
    refused("clip_state must be fp32", dc, dst, theta, x, 0.5, f(4, bf), None)
    refused("clip_state must be on the GPU", dc, dst, theta, x, 0.5,
            state.cpu(), None)
    refused("w_out must be fp32", dc, dst, theta, x, 0.5, state, f(8, bf))
    refused("alpha must not be NaN", dc, dst, theta, x, math.nan, state, None)
    # fedopt_finalize
    refused("round_state must have 4 elements", ops.fedopt_finalize, f(4),
            f(8))
    refused("round_state must be fp32", ops.fedopt_finalize, f(4), f(4, bf))
    refused("w_sum must be on the GPU", ops.fedopt_finalize, f(4).cpu(), state)
    # server_step
    D, m, v, rs = f(64), f(64), f(64), f(4)

    def step(mode="fedadam", D=D, x=x, m=m, v=v, lr=0.1, b1=0.9, b2=0.99,
             tau=1e-3, rs=rs):
        ops.server_step(mode, D, x, m, v, lr, b1, b2, tau, rs)

    kw = lambda **k: (lambda: step(**k))
    refused("unknown mode", kw(mode="fedlion"))
    refused("D must be fp32", kw(D=f(64, bf)))
    refused("D must have 64 elements", kw(D=f(68)))
    refused("x must be contiguous", kw(x=f(128)[::2]))
    refused("m must be 16-byte aligned", kw(m=f(65)[1:]))
    refused("m is undefined", kw(mode="fedavgm", m=None))
    refused("v is undefined", kw(v=None))
    refused("v must be fp32", kw(v=f(64, bf)))
    refused("v must be on the GPU", kw(v=f(64).cpu()))
    refused("round_state must have 4 elements", kw(rs=f(5)))
    refused("round_state must be fp32", kw(rs=f(4, bf)))
    for bad in (0.0, -1.0, math.nan):
        refused("lr must be > 0", kw(lr=bad))
        refused("tau must", kw(tau=bad))
    for bad in (-0.1, 1.0, math.nan):
        refused(r"beta1 must be in \[0, 1\)", kw(b1=bad))
        refused(r"beta2 must be in \[0, 1\)", kw(b2=bad))
    refused("tau must not be NaN", kw(mode="fedavgm", tau=math.nan))
    torch.cuda.synchronize()
    for t in (dst, D, m, v, rs, state, partials):
        assert not t.any()                           # nothing was launched
    step(mode="fedavgm", v=None, tau=0.0)            # tau is the adaptive modes'
    step(mode="mean", m=None, v=None)


# ---- RCCL, world 1 -------------------------------------------------------------

def _nccl_world1_main():
    """Runs in a fresh process (see test_nccl_world1_fedopt)."""
    from collections import OrderedDict

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29915",
                      RANK="0", WORLD_SIZE="1")
    from baton_amd.fed.server_opt import ServerOptimizer
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    native_ops()
    nn = torch.nn
    plane = FederatedDataPlane(DataPlaneConfig(backend="nccl"),
                               device=torch.device("cuda", 0))
    assert plane._side_stream is not None

    # -- three rounds of fedadam with clipping, then a poisoned round
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(64, 128), nn.BatchNorm1d(128),
                          nn.Linear(128, 32)).to("cuda").bfloat16()
    model.train()
    model(torch.randn(8, 64, device="cuda").bfloat16())
    arena = FlatParamArena(model)
    names = [f"g{i}" for i in range(len(arena.all_groups))]
    cfg = ServerOptConfig(name="fedadam", lr=HP["lr"], beta1=HP["b1"],
                          beta2=HP["b2"], tau=HP["tau"], client_clip_norm=1.0)
    plane.enable_server_opt(arena, cfg)
    oracle = ServerOptimizer("fedadam", HP["lr"], HP["b1"], HP["b2"],
                             HP["tau"], 1.0)
    flats = lambda: OrderedDict(
        (k, g.flat.detach().cpu().clone())
        for k, g in zip(names, arena.all_groups))
    T = max(chain_of(g.flat.numel(), 8) for g in arena.all_groups)
    rD = E + 2 * (E + COEF_BOUND + norm_bound(T))
    n_param_groups = len(arena.groups)

    def sync_oracle(state):
        for i, k in enumerate(names):
            oracle.x[k] = state[f"x.{i}"].clone()
            if f"m.{i}" in state:
                oracle.m[k] = state[f"m.{i}"].clone()
                oracle.v[k] = state[f"v.{i}"].clone()

    worst = 0.0
    for rnd in range(3):
        gen = torch.Generator().manual_seed(50 + rnd)
        for g in arena.all_groups:              # the client's local training
            noise = 0.05 * torch.randn(g.flat.numel(), generator=gen)
            g.flat.add_(noise.to(g.flat.device, g.flat.dtype))
        before = plane.server_opt_state()
        client = flats()
        sync_oracle(before)
        plane.fedopt_arena(arena, 123, async_handle=True)
        w = plane.pending.wait()
        torch.cuda.synchronize()
        assert w.tolist() == [123.0]
        after = plane.server_opt_state()
        global_sd = OrderedDict((k, t.clone()) for k, t in client.items())
        oracle.step_(global_sd, [client], [123.0], names[:n_param_groups])
        cs = plane.fedopt_clip_state.tolist()
        assert cs[2] == 1.0 and cs[1] < 1.0, cs      # clipped
        # the oracle's own norm: float64 over the rounded differences (e)
        assert abs(cs[0] / oracle.norm[0] - 1.0) <= norm_bound(T) + E
        assert abs(cs[1] / oracle.coef[0] - 1.0) <= 2 * (COEF_BOUND
                                                         + norm_bound(T))
        assert after["round_state"].tolist() == [1.0, 1.0, 1.0, 0.0]
        for i, k in enumerate(names):
            mode = "fedadam" if i < n_param_groups else "mean"
            z = np.zeros(before[f"x.{i}"].numel(), np.float32)
            ins = [before.get(f"{s}.{i}") for s in "xmv"]
            ins = [z if a is None else a.numpy() for a in ins]
            out = {s: after[f"{s}.{i}"].numpy() for s in "xmv"
                   if f"{s}.{i}" in after}
            ref = step_ref(mode, oracle.last_D[k].numpy(), 1.0, *ins, rD=rD)
            for s in out:
                worst = max(worst, worst_ratio(out[s], *ref[s]))
            # every rank installs bf16(x)
            g = arena.all_groups[i]
            assert same_bits(g.flat.detach().cpu(),
                             after[f"x.{i}"].to(g.flat.dtype))
        print(f"round {rnd}: norm {cs[0]:.4f} coef {cs[1]:.4f}, worst "
              f"{worst:.3f} of the bound")
        assert worst <= 1.0
    assert arena.check_views()

    before = plane.server_opt_state()
    with torch.no_grad():
        model[0].weight[3, 5] = math.inf
    plane.fedopt_arena(arena, 123)
    torch.cuda.synchronize()
    after = plane.server_opt_state()
    assert after["round_state"].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert plane.fedopt_clip_state.tolist()[1:] == [0.0, 0.0, 1.0]
    for k in before:
        if k != "round_state":
            assert same_bits(before[k], after[k]), k
    for i, g in enumerate(arena.all_groups):
        assert torch.isfinite(g.flat).all()
        assert same_bits(g.flat.detach().cpu(),
                         after[f"x.{i}"].to(g.flat.dtype))

    # -- the fp32 master: two updates of less than half a bf16 ulp add up
    lin = nn.Linear(16, 8).to("cuda").bfloat16()
    with torch.no_grad():
        lin.weight.fill_(1.0)
        lin.bias.fill_(1.0)
    arena2 = FlatParamArena(lin)
    plane.enable_server_opt(arena2, ServerOptConfig(
        name="fedavgm", lr=0.4, beta1=0.0))
    ulp = 2.0 ** -7
    flat = arena2.groups[0].flat
    seen = []
    for rnd in range(2):
        flat.fill_(1.0 + ulp)                   # the client moves one ulp up
        plane.fedopt_arena(arena2, 7)
        torch.cuda.synchronize()
        seen.append((plane.server_opt_state()["x.0"].clone(),
                     flat.detach().float().cpu().clone()))
    (x1, t1), (x2, t2) = seen
    assert (x1 > 1.0).all() and (x1 < 1.0 + 0.5 * ulp).all()
    assert (t1 == 1.0).all()                    # below half an ulp: not yet
    assert (x2 > 1.0 + 0.5 * ulp).all() and (x2 - x1 < 0.5 * ulp).all()
    assert (t2 == 1.0 + ulp).all()              # the second one shows in bf16
    plane.shutdown()
    print("FEDOPT-NCCL-1RANK-OK")


@pytest.mark.gpu
def test_nccl_world1_fedopt():
    native_ops()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here])
    code = "import test_fedopt_exact as t; t._nccl_world1_main()"
    proc = subprocess.run([sys.executable, "-c", code], env=env,
                          capture_output=True, text=True, timeout=300)
    print(proc.stdout[-3000:])
    assert proc.returncode == 0, (
        f"nccl world-1 fedopt failed:\n{proc.stdout[-2000:]}\n"
        f"{proc.stderr[-4000:]}")
    assert "FEDOPT-NCCL-1RANK-OK" in proc.stdout

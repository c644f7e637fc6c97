"""DP noise on the device (ops/csrc/fedopt.hip: dp_noise_kernel and
server_step_kernel<MODE, true>) against the float64 oracle of
fed/server_opt.py, and ``fedopt_arena`` with noise on RCCL at world 1.

Notation: e = 2^-24, one fp32 rounding; K = 1 + 2^-10 covers second-order
terms. The threshold is 1.0 of each bound below; nothing is fitted.

The normal. u1, u2 and t = 2 u2 are exact in fp32. The device forms
L = logf(u1) (A_log ulp, i.e. at most 2 A_log e relative), p = fl(-2 L)
(exact), R = sqrtf(p) (correctly rounded, as the other exact tests take it:
the square root halves the error of p and rounds once, A_log e + e),
c = cospif(t) or sinpif(t) (A_trig ulp, 2 A_trig e relative) and
zeta = fl(R c) (e):

    |zeta - ref| <= K (A_log + 2 A_trig + 2) e |ref| + 2^-50

No copy of the device math library's accuracy table is on hand, so A_log = 3
and A_trig = 4 are the OpenCL full-profile conformance limits for log and
sinpi / cospi (OpenCL C specification, "Relative error as ULPs"), which every
conforming implementation meets. The absolute term covers the exact zeros of
cospi and sinpi; the oracle reduces the argument by quadrant, so its zeros are
exact too. With sigma = 1, xi = fl(1 zeta) is zeta itself; any other sigma is
one more rounding, checked for bits against torch's fp32 product.

The fused step. xi^ = fl(sigma zeta^) and Delta^ = fl(D + xi^) against
Delta = D + sigma zeta_ref in float64 from the stored D:

    dxi    = K (A_log + 2 A_trig + 3) e |xi| + sigma 2^-50
    dDelta = dxi + e |Delta|

The sum can cancel, so the error of Delta^ is not relative to Delta with a
fixed constant: the bounds of tests/test_fedopt_exact.py are taken with rD,
their relative error of Delta^, replaced elementwise by dDelta / |Delta| (its
one rounding e plus dxi / |Delta|). Those bounds are first order in rD with K
for the rest, which holds while rD <= 2^-9; the tests assert that of their
(deterministic) inputs. inv_W is not part of the definition: the reference
never multiplies by it, and the device's round_state holds inv_W = 4/3, so a
kernel that did would be far outside.

A slice call (the data plane's buckets) at elem_offset = 4096 equals the
matching slice of a whole-buffer call for bits, and server_step_noise with
sigma = 0 and W = 1 (Delta = D + 0) equals ``ops.server_step`` with W = 1
(Delta = D 1) for bits: the noise-off kernel is the one it always was.

World-1 RCCL. ``fedopt_arena`` with z = 1 against ``ServerOptimizer`` with the
same seed, group ordinals as streams on both sides. D^ meets the composition
of the existing world-1 test, rD0 = e + 2 (e + 2^-22 + norm bound), relative
to the oracle's D; sigma is the same fp32 number on both sides, so

    dDelta = rD0 |D| + dxi + e |Delta|

The unmarked tests emulate the index walk and the fp32 arithmetic in numpy
(logarithm and trigonometry correctly rounded from float64): honest arithmetic
meets every bound, and each single defect exceeds 4x or fails an equality."""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fedopt_exact import (  # noqa: E402
    COEF_BOUND, DEV, E, HP, K2, MODES, canaries_alive, chain_of,
    emu_round_state, emu_server_step, gpu_round_state, in_parent, native_ops,
    norm_bound, same_bits, same_bits_np, step_inputs, step_ref, worst_ratio,
)

from baton_amd.fed.server_opt import philox4x32, unit_normals  # noqa: E402

A_LOG, A_TRIG = 3, 4
ZETA_REL = K2 * (A_LOG + 2 * A_TRIG + 2) * E
XI_REL = K2 * (A_LOG + 2 * A_TRIG + 3) * E
ABS = 2.0 ** -50
RD_MAX = 2.0 ** -9
SEED = 0xC0FFEE0DDBA11AD5
FAR = 4 * (2 ** 32 - 1)
NOISE_SIZES = [1, 3, 4, 5, 1023, 4097, 4194333]
STEP_SIZES = [1, 3, 4, 5, 1023, 1024 * 4 + 1]
SLICE_AT = 4096
SIGMA = 0.25
W, INV_W = 0.75, float(np.float32(1.0 / 0.75))


@functools.lru_cache(maxsize=None)
def oracle(n, rnd, stream, offset):
    z = unit_normals(SEED, rnd, stream, offset, n)
    z.setflags(write=False)
    return z


def zeta_ratio(got, ref):
    return worst_ratio(got, ref, ZETA_REL * np.abs(ref) + ABS)


def noised_ref(mode, D, x0, m0, v0, xi_ref, sigma, rD0=0.0):
    """(reference, bound) per output of one noised step, with rD elementwise
    (the docstring); also the largest rD."""
    delta = np.asarray(D, np.float64) + xi_ref
    dxi = XI_REL * np.abs(xi_ref) + sigma * ABS
    ddelta = rD0 * np.abs(np.asarray(D, np.float64)) + dxi + E * np.abs(delta)
    with np.errstate(divide="ignore", invalid="ignore"):
        rD = np.where(delta != 0, ddelta / np.abs(delta), 0.0)
    return step_ref(mode, delta, 1.0, x0, m0, v0, rD=rD), float(rD.max())


def noised_ratios(mode, out, D, x0, m0, v0, xi_ref, sigma, rD0=0.0):
    ref, rmax = noised_ref(mode, D, x0, m0, v0, xi_ref, sigma, rD0)
    assert rmax <= RD_MAX, f"cancellation beyond first order: rD {rmax}"
    return {k: worst_ratio(out[k], *ref[k]) for k in ref}


# ---- numpy emulation of the kernels ------------------------------------------

def trig64(t):
    """(cospi(t), sinpi(t)) for t in [0, 2), reduced by quadrant."""
    q = np.floor(2.0 * t)
    r = t - 0.5 * q
    c, s = np.cos(np.pi * r), np.sin(np.pi * r)
    return (np.select([q == 0, q == 1, q == 2], [c, -s, -c], s),
            np.select([q == 0, q == 1, q == 2], [s, c, -s], -c))


def emu_box_muller(a, b):
    u1 = ((a >> np.uint32(8)) + np.uint32(1)).astype(np.float32) \
        * np.float32(2.0 ** -24)
    u2 = (b >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    L = np.log(u1.astype(np.float64)).astype(np.float32)
    R = np.sqrt(np.float32(-2.0) * L)
    c, s = trig64((np.float32(2.0) * u2).astype(np.float64))
    return R * c.astype(np.float32), R * s.astype(np.float32)


def emu_zeta(n, rnd, stream, elem_offset, swap_lanes=False, r0_twice=False,
             drop_hi=False, tail_block0=False, ignore_offset=False):
    """The fp32 normals of an n-element launch: one block per f32x4, the
    tail from block (elem_offset + n) >> 2."""
    off = 0 if ignore_offset else elem_offset
    nvec = n // 4
    j = (off >> 2) + np.arange(nvec + (1 if n % 4 else 0)).astype(np.uint64)
    if tail_block0 and n % 4:
        j[-1] = 0
    lo, hi = j & np.uint64(0xFFFFFFFF), j >> np.uint64(32)
    r = philox4x32((lo, 0 * hi if drop_hi else hi, rnd, stream),
                   (SEED & 0xFFFFFFFF, SEED >> 32))
    z = np.stack(emu_box_muller(r[0], r[0] if r0_twice else r[1])
                 + emu_box_muller(r[2], r[2] if r0_twice else r[3]), axis=1)
    if swap_lanes:
        z = z[:, [1, 0, 3, 2]]
    return np.ascontiguousarray(z.reshape(-1)[:n])


def emu_noised_step(mode, ins, rs, rnd, stream, elem_offset, sigma,
                    times_inv_w=False, **defects):
    D, x0, m0, v0 = ins
    if rs[2] == 0.0:
        return {"x": x0, "m": m0, "v": v0}
    xi = np.float32(sigma) * emu_zeta(D.size, rnd, stream, elem_offset,
                                      **defects)
    delta = D + xi
    one = rs.copy()
    if not times_inv_w:
        one[1] = 1.0
    return emu_server_step(mode, delta, x0, m0, v0, one)


def test_emulated_normals_meet_the_bound():
    for n in NOISE_SIZES[:-1] + [70001]:
        for off in (0, 4) + ((FAR,) if n <= 1023 else ()):
            for rnd, stream in ((0, 0), (7, 3)):
                r = zeta_ratio(emu_zeta(n, rnd, stream, off),
                               oracle(n, rnd, stream, off))
                print(f"emu zeta n={n} off={off} t={rnd} s={stream}: {r:.3f}")
                assert r <= 1.0
    # the exact zeros of cospi and sinpi
    b = np.asarray([0, 1, 2, 3], np.uint32) << np.uint32(30)
    c, s = emu_box_muller(np.full(4, 0xDEADBEEF, np.uint32), b)
    assert c[1] == 0 and c[3] == 0 and s[0] == 0 and s[2] == 0
    # u1 = 1: R = 0
    c, s = emu_box_muller(np.full(4, 0xFFFFFF00, np.uint32), b)
    assert not c.any() and not s.any()


@pytest.mark.parametrize("mode", MODES)
def test_emulated_noised_step_meets_the_bound(mode):
    rs = emu_round_state(W)
    assert rs[1] == np.float32(INV_W)
    for n in STEP_SIZES:
        ins = step_inputs(n, 1.0)
        out = emu_noised_step(mode, ins, rs, 5, 2, 0, SIGMA)
        xi_ref = float(np.float32(SIGMA)) * oracle(n, 5, 2, 0)
        r = noised_ratios(mode, out, *ins, xi_ref, SIGMA)
        print(f"emu noised {mode} n={n}: {r}")
        assert max(r.values()) <= 1.0
    # the bucket path: a slice at SLICE_AT is the whole buffer's slice
    n = SLICE_AT + 1023
    ins = step_inputs(n, 1.0)
    whole = emu_noised_step(mode, ins, rs, 5, 2, 0, SIGMA)
    part = emu_noised_step(mode, tuple(a[SLICE_AT:] for a in ins), rs, 5, 2,
                           SLICE_AT, SIGMA)
    for k in "xmv":
        assert same_bits_np(part[k], whole[k][SLICE_AT:])


def test_single_defects_exceed_4x_or_fail_an_equality():
    n = 1023
    ref = oracle(n, 7, 3, 0)
    assert zeta_ratio(emu_zeta(n, 7, 3, 0), ref) <= 1.0
    # lanes swapped, r0 for both uniforms, the tail from block 0
    assert zeta_ratio(emu_zeta(n, 7, 3, 0, swap_lanes=True), ref) > 4.0
    assert zeta_ratio(emu_zeta(n, 7, 3, 0, r0_twice=True), ref) > 4.0
    assert zeta_ratio(emu_zeta(n, 7, 3, 0, tail_block0=True), ref) > 4.0
    assert zeta_ratio(emu_zeta(5, 7, 3, 4, tail_block0=True),
                      oracle(5, 7, 3, 4)) > 4.0
    # hi32(j) dropped: only beyond 2^32 blocks
    assert zeta_ratio(emu_zeta(n, 7, 3, 0, drop_hi=True), ref) <= 1.0
    assert zeta_ratio(emu_zeta(5, 7, 3, FAR), oracle(5, 7, 3, FAR)) <= 1.0
    assert zeta_ratio(emu_zeta(5, 7, 3, FAR, drop_hi=True),
                      oracle(5, 7, 3, FAR)) > 4.0
    # the bucket offset ignored: the slice is no longer the whole's slice
    rs = emu_round_state(W)
    n = SLICE_AT + 1023
    ins = step_inputs(n, 1.0)
    tail = tuple(a[SLICE_AT:] for a in ins)
    whole = emu_noised_step("fedadam", ins, rs, 5, 2, 0, SIGMA)
    part = emu_noised_step("fedadam", tail, rs, 5, 2, SLICE_AT, SIGMA,
                           ignore_offset=True)
    assert not same_bits_np(part["x"], whole["x"][SLICE_AT:])
    xi_ref = float(np.float32(SIGMA)) * oracle(1023, 5, 2, SLICE_AT)
    assert max(noised_ratios("fedadam", part, *tail, xi_ref,
                             SIGMA).values()) > 4.0
    # inv_W multiplied in
    xi_ref = float(np.float32(SIGMA)) * oracle(n, 5, 2, 0)
    for mode in MODES:
        good = emu_noised_step(mode, ins, rs, 5, 2, 0, SIGMA)
        assert max(noised_ratios(mode, good, *ins, xi_ref,
                                 SIGMA).values()) <= 1.0
        bad = emu_noised_step(mode, ins, rs, 5, 2, 0, SIGMA, times_inv_w=True)
        assert max(noised_ratios(mode, bad, *ins, xi_ref,
                                 SIGMA).values()) > 4.0
    # the round not advanced on a skip: applied, skipped, applied
    ins = step_inputs(1023, 1.0)
    skip = emu_round_state(0.0)
    for advance_on_skip in (True, False):
        t, state = 0, ins
        for r in (rs, skip, rs):
            out = emu_noised_step("fedavgm", state, r, t, 0, 0, SIGMA)
            applied = r[2] != 0.0
            if not applied:
                assert all(same_bits_np(out[k], a)
                           for k, a in zip("xmv", state[1:]))
            last_in, last_t = state, t
            state = (ins[0], out["x"], out["m"], out["v"])
            t += 1 if (applied or advance_on_skip) else 0
        xi_ref = float(np.float32(SIGMA)) * oracle(1023, 2, 0, 0)
        worst = max(noised_ratios("fedavgm", out, *last_in, xi_ref,
                                  SIGMA).values())
        assert (last_t == 2 and worst <= 1.0) if advance_on_skip \
            else (last_t == 1 and worst > 4.0)


# ---- GPU ---------------------------------------------------------------------

def gpu_noise(ops, n, rnd, stream, offset, sigma=1.0):
    parent, out = in_parent(torch.zeros(n))
    ops.dp_noise(out, SEED, rnd, stream, offset, sigma)
    assert canaries_alive(parent)
    return out


# only the small sizes run at the large offset
NOISE_CASES = [(n, off) for n in NOISE_SIZES for off in (0, 4, FAR)
               if off != FAR or n <= 1023]


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", NOISE_CASES)
def test_dp_noise_against_the_oracle(n, offset):
    ops = native_ops()
    for rnd, stream in ((0, 0), (7, 3)):
        out = gpu_noise(ops, n, rnd, stream, offset)
        r = zeta_ratio(out.cpu().numpy(), oracle(n, rnd, stream, offset))
        print(f"dp_noise n={n} off={offset} t={rnd} s={stream}: "
              f"{r:.3f} of the bound")
        assert r <= 1.0
        assert same_bits(out, gpu_noise(ops, n, rnd, stream, offset))
    a, b = gpu_noise(ops, n, 0, 0, offset), gpu_noise(ops, n, 0, 3, offset)
    c = gpu_noise(ops, n, 7, 0, offset)
    assert not same_bits(a, b) and not same_bits(a, c)
    # any other sigma is one fp32 product more
    s = torch.tensor(0.37, dtype=torch.float32, device=DEV)
    assert same_bits(gpu_noise(ops, n, 0, 0, offset, 0.37), s * a)
    assert not gpu_noise(ops, n, 0, 0, offset, 0.0).any()


def gpu_noised_step(ops, mode, ins, rs, rnd, stream, offset, sigma):
    D, x0, m0, v0 = ins
    parents = [in_parent(a) for a in (D, x0, m0, v0)]
    (_, Dv), (_, xv), (_, mv), (_, vv) = parents
    ops.server_step_noise(mode, Dv, xv, mv if mode != "mean" else None,
                          vv if mode in MODES[2:] else None, HP["lr"],
                          HP["b1"], HP["b2"], HP["tau"], rs, SEED, rnd, stream,
                          offset, sigma)
    for p, _ in parents:
        assert canaries_alive(p)
    assert same_bits(Dv, torch.from_numpy(D).to(DEV))
    return {"x": xv.cpu().numpy(), "m": mv.cpu().numpy(),
            "v": vv.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_noised_step_against_float64(mode):
    ops = native_ops()
    rs = gpu_round_state(ops, W)
    assert rs.tolist() == [W, INV_W, 1.0, 0.0]
    for n in STEP_SIZES:
        ins = step_inputs(n, 1.0)
        out = gpu_noised_step(ops, mode, ins, rs, 5, 2, 0, SIGMA)
        xi_ref = float(np.float32(SIGMA)) * oracle(n, 5, 2, 0)
        r = noised_ratios(mode, out, *ins, xi_ref, SIGMA)
        print(f"noised {mode} n={n}: {r} of the bounds")
        assert max(r.values()) <= 1.0
        if mode in ("mean", "fedavgm"):
            assert same_bits_np(out["v"], ins[3])
        if mode == "mean":
            assert same_bits_np(out["m"], ins[2])
    # a bucket: the slice at SLICE_AT against float64 and the whole buffer
    n = SLICE_AT + 1023
    ins = step_inputs(n, 1.0)
    tail = tuple(np.ascontiguousarray(a[SLICE_AT:]) for a in ins)
    whole = gpu_noised_step(ops, mode, ins, rs, 5, 2, 0, SIGMA)
    part = gpu_noised_step(ops, mode, tail, rs, 5, 2, SLICE_AT, SIGMA)
    xi_ref = float(np.float32(SIGMA)) * oracle(1023, 5, 2, SLICE_AT)
    assert max(noised_ratios(mode, part, *tail, xi_ref, SIGMA).values()) <= 1.0
    for k in "xmv":
        assert same_bits_np(part[k], whole[k][SLICE_AT:])


@pytest.mark.gpu
def test_skipped_round_with_noise_keeps_every_bit():
    ops = native_ops()
    ins = step_inputs(256 * 4 + 1, 1.0)
    rs = gpu_round_state(ops, 0.0)
    assert rs.tolist()[1:] == [0.0, 0.0, 1.0]
    for mode in MODES:
        out = gpu_noised_step(ops, mode, ins, rs, 5, 2, 0, SIGMA)
        for k, a in zip("xmv", ins[1:]):
            assert same_bits_np(out[k], a)


@pytest.mark.gpu
def test_noise_off_is_the_step_it_was():
    ops = native_ops()
    rs = gpu_round_state(ops, 1.0)
    for n in (5, 1024 * 4 + 1):
        ins = step_inputs(n, 1.0)
        for mode in MODES:
            parents = [in_parent(a) for a in ins]
            (_, Dv), (_, xv), (_, mv), (_, vv) = parents
            ops.server_step(mode, Dv, xv, mv if mode != "mean" else None,
                            vv if mode in MODES[2:] else None, HP["lr"],
                            HP["b1"], HP["b2"], HP["tau"], rs)
            off = gpu_noised_step(ops, mode, ins, rs, 5, 2, 0, 0.0)
            for k, t in (("x", xv), ("m", mv), ("v", vv)):
                assert same_bits_np(off[k], t.cpu().numpy()), (mode, n, k)


@pytest.mark.gpu
def test_noise_refusals():
    ops = native_ops()
    f = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    D, x, m, v, rs, out = f(64), f(64), f(64), f(64), f(4), f(64)
    rs[2] = 1.0

    def step(seed=SEED, rnd=0, stream=0, offset=0, sigma=1.0, mode="fedadam",
             D=D):
        ops.server_step_noise(mode, D, x, m, v, 0.1, 0.9, 0.99, 1e-3, rs, seed,
                              rnd, stream, offset, sigma)

    def noise(out=out, seed=SEED, rnd=0, stream=0, offset=0, sigma=1.0):
        ops.dp_noise(out, seed, rnd, stream, offset, sigma)

    for fn in (step, noise):
        for bad in (1, 2, 3, 6, -4):
            with pytest.raises(RuntimeError, match="elem_offset must be"):
                fn(offset=bad)
        for bad in (-1, 2 ** 32):
            with pytest.raises(RuntimeError, match="stream must be in"):
                fn(stream=bad)
        for bad in (-1.0, math.inf, math.nan):
            with pytest.raises(RuntimeError, match="sigma must be finite"):
                fn(sigma=bad)
        with pytest.raises(RuntimeError, match="round must be >= 0"):
            fn(rnd=-1)
        for bad in (-1, 2 ** 64):
            with pytest.raises(TypeError):
                fn(seed=bad)
    with pytest.raises(RuntimeError, match="unknown mode"):
        step(mode="fedlion")
    with pytest.raises(RuntimeError, match="server_step_noise: D must be fp32"):
        step(D=f(64, torch.bfloat16))
    with pytest.raises(RuntimeError, match="out must be fp32"):
        noise(out=f(64, torch.bfloat16))
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        noise(out=f(65)[1:])
    with pytest.raises(RuntimeError, match="out must be on the GPU"):
        noise(out=f(64).cpu())
    torch.cuda.synchronize()
    for t in (D, x, m, v, out):
        assert not t.any()                           # nothing was launched
    noise(stream=2 ** 32 - 1, seed=2 ** 64 - 1, offset=FAR)
    step(stream=2 ** 32 - 1, seed=0)
    torch.cuda.synchronize()
    assert out.any() and x.any()


# ---- RCCL, world 1 -------------------------------------------------------------

def _nccl_world1_main():
    """Runs in a fresh process (see test_nccl_world1_fedopt_with_noise)."""
    from collections import OrderedDict

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29916",
                      RANK="0", WORLD_SIZE="1")
    from baton_amd.fed.server_opt import ServerOptimizer, f32 as sf32
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    native_ops()
    nn = torch.nn
    plane = FederatedDataPlane(DataPlaneConfig(backend="nccl"),
                               device=torch.device("cuda", 0))
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(64, 128), nn.BatchNorm1d(128),
                          nn.Linear(128, 32)).to("cuda").bfloat16()
    model.train()
    model(torch.randn(8, 64, device="cuda").bfloat16())
    arena = FlatParamArena(model)
    names = [f"g{i}" for i in range(len(arena.all_groups))]
    z, clip = 1.0, 1.0
    cfg = ServerOptConfig(name="fedadam", lr=HP["lr"], beta1=HP["b1"],
                          beta2=HP["b2"], tau=HP["tau"], client_clip_norm=clip,
                          dp_noise_multiplier=z, dp_seed=SEED)
    plane.enable_server_opt(arena, cfg)
    oracle_opt = ServerOptimizer("fedadam", HP["lr"], HP["b1"], HP["b2"],
                                 HP["tau"], clip, noise_multiplier=z,
                                 seed=SEED)
    sigma = sf32(z * clip * 1.0)
    flats = lambda: OrderedDict(
        (k, g.flat.detach().cpu().clone())
        for k, g in zip(names, arena.all_groups))
    T = max(chain_of(g.flat.numel(), 8) for g in arena.all_groups)
    rD0 = E + 2 * (E + COEF_BOUND + norm_bound(T))
    n_param_groups = len(arena.groups)

    def train(rnd):
        gen = torch.Generator().manual_seed(50 + rnd)
        for g in arena.all_groups:
            noise = 0.05 * torch.randn(g.flat.numel(), generator=gen)
            g.flat.add_(noise.to(g.flat.device, g.flat.dtype))

    worst = 0.0
    for rnd in range(2):
        train(rnd)
        before = plane.server_opt_state()
        assert int(before["dp_rounds"]) == rnd == plane.dp_rounds
        client = flats()
        for i, k in enumerate(names):
            oracle_opt.x[k] = before[f"x.{i}"].clone()
            if f"m.{i}" in before:
                oracle_opt.m[k] = before[f"m.{i}"].clone()
                oracle_opt.v[k] = before[f"v.{i}"].clone()
        plane.fedopt_arena(arena, 123)
        torch.cuda.synchronize()
        after = plane.server_opt_state()
        assert int(after["dp_rounds"]) == rnd + 1
        assert after["round_state"].tolist() == [1.0, 1.0, 1.0, 0.0]
        global_sd = OrderedDict((k, t.clone()) for k, t in client.items())
        assert oracle_opt.dp_rounds == rnd
        oracle_opt.step_(global_sd, [client], [123.0], names[:n_param_groups])
        assert oracle_opt.last_sigma == sigma
        for i, k in enumerate(names):
            mode = "fedadam" if i < n_param_groups else "mean"
            n = before[f"x.{i}"].numel()
            zero = np.zeros(n, np.float32)
            ins = [before.get(f"{s}.{i}") for s in "xmv"]
            ins = [zero if a is None else a.numpy() for a in ins]
            out = {s: after[f"{s}.{i}"].numpy() for s in "xmv"
                   if f"{s}.{i}" in after}
            xi_ref = sigma * unit_normals(SEED, rnd, i, 0, n)
            ref, rmax = noised_ref(mode, oracle_opt.last_D[k].numpy(), *ins,
                                   xi_ref, sigma, rD0=rD0)
            assert rmax <= RD_MAX
            for s in out:
                worst = max(worst, worst_ratio(out[s], *ref[s]))
            # the oracle's own step lies within the same bound
            assert worst_ratio(oracle_opt.x[k].numpy(), *ref["x"]) <= 1.0
            g = arena.all_groups[i]
            assert same_bits(g.flat.detach().cpu(),
                             after[f"x.{i}"].to(g.flat.dtype))
        print(f"round {rnd}: worst {worst:.3f} of the bound")
        assert worst <= 1.0

    # the round after a restore is the uninterrupted run's, for bits
    saved = plane.server_opt_state()
    train(2)
    sent = [g.flat.detach().clone() for g in arena.all_groups]
    plane.fedopt_arena(arena, 123)
    torch.cuda.synchronize()
    straight = plane.server_opt_state()
    assert int(straight["dp_rounds"]) == 3
    plane.load_server_opt_state(saved)
    assert plane.dp_rounds == 2
    for g, t in zip(arena.all_groups, sent):
        g.flat.copy_(t)
    plane.fedopt_arena(arena, 123)
    torch.cuda.synchronize()
    resumed = plane.server_opt_state()
    assert list(resumed) == list(straight)
    for k in straight:
        if straight[k].dtype == torch.float32:
            assert same_bits(straight[k], resumed[k]), k
        else:
            assert torch.equal(straight[k], resumed[k]), k
    # without the restored counter it is another draw
    plane.load_server_opt_state(saved)
    plane._fedopt["dp_rounds"] = 0
    for g, t in zip(arena.all_groups, sent):
        g.flat.copy_(t)
    plane.fedopt_arena(arena, 123)
    torch.cuda.synchronize()
    assert not same_bits(plane.server_opt_state()["x.0"], straight["x.0"])
    plane.shutdown()
    print("DP-NCCL-1RANK-OK")


@pytest.mark.gpu
def test_nccl_world1_fedopt_with_noise():
    native_ops()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here])
    code = "import test_dp_noise_exact as t; t._nccl_world1_main()"
    proc = subprocess.run([sys.executable, "-c", code], env=env,
                          capture_output=True, text=True, timeout=300)
    print(proc.stdout[-3000:])
    assert proc.returncode == 0, (
        f"nccl world-1 fedopt with noise failed:\n{proc.stdout[-2000:]}\n"
        f"{proc.stderr[-4000:]}")
    assert "DP-NCCL-1RANK-OK" in proc.stdout

"""The streaming kernels (elementwise.hip, llama_ops.hip, fedmath.hip, the MSE
kernels of loss.hip) in fp32 and bf16 against float64 built from the *stored*
inputs, with elementwise bounds that have no free constant and a threshold of
1.0 (the form of tests/test_softmax_exact.py and tests/test_ce_exact.py).

Notation: e = 2^-24 is one fp32 rounding, u = 2^-8 one round-to-nearest-even
bf16 store, store = u (bf16) or 0 (fp32), tiny = 2^-126 the smallest normal
fp32. Every bound is ``store |ref| + F * (fp32 term)``; F = 1 + u carries the
(1 + u) of storing an already rounded value and every second-order product of
the first-order terms (the largest first-order term below is a few hundred e,
so its square is far under u times it). Scalars (alpha, dout, a, b) enter the
reference as the float32 the kernel receives, as do the GELU constants.

Exact ops, compared bit for bit: ``relu_fwd`` (x where x > 0, else a zero of
either sign), ``relu_bwd`` (dy where y > 0, else 0, also where that dy is
NaN: it selects, it does not multiply), ``scale_fwd`` / ``scale_cast`` with
alpha a power of two or 1, ``cast_copy<float>``, ``cast_copy<bf16>`` against
torch's CPU conversion on a table of special values, ``transpose2d``.

One-rounding ops (fp32 term):

    add_relu    e |a + b|          the add; relu is monotone and 1-Lipschitz
    add_scaled  e |ref|            one fma
    scale       e |ref|
    scale_cast  e |ref|            store = 0, the output is fp32
    axpby       e |b y| + e |ref|  fl(b y), then one fma
    mse_bwd     3 e |ref|          2 dout is exact and n < 2^24 converts
                                   exactly: the division, x - y, the multiply

SwiGLU. ``__expf(-a)`` is taken as test_softmax_exact.py takes it: the argument
scaling moves exp by 2 |a| e, exp2 is good to 1 ulp = 2 e. With sig the true
sigmoid, 1 + exp rounds once and the reciprocal is good to 1 ulp:

    dsig = ((1 - sig) (2 |a| + 2) + 3) e             relative error of sig
    y, db:  |ref| (dsig + 2 e)                       two more multiplies
    da:     |dy b| (sig dsig (|g| + |a| sig) + e sig |a| (1 - sig)
                    + 2 e sig |g|) + 2 e |ref|,      g = 1 + a (1 - sig)

In da the kernel forms 1 - sig from its own sig: the error sig dsig of sig is
an *absolute* error of 1 - sig, however small 1 - sig is (large positive a),
and the fma a (1 - sig) + 1 carries it times |a|. Where exp(-a) overflows
(a <= -89) sig is 0 instead of a number below tiny: tiny (|a b| + 1) for y,
tiny (|dy a| + 1) for db and tiny (|dy b| (1 + |a|) + 1) for da cover that and
any result below the normal range; y is a zero there, never NaN.

GELU, w = v + k v^3, inner = c0 w, t = tanh(inner): k v, (k v) v and the fma
give 2 e k |v|^3 + e |w|, the multiply by c0 one more e:

    dI = 2 e c0 k |v|^3 + 2 e |inner|
    dT = (1 - t^2) dI + 10 e |t|             tanhf at 5 ulp of its result
    y:   0.5 |v| (dT + e (1 + t)) + e |ref|

Near t -> -1 the sum 1 + t cancels, so the tanh error is an absolute error of
the result, 0.5 |v| dT. The backward, grad = A + B with A = 0.5 (1 + t),
q = 1 - t^2 (cancels too), D = c0 (1 + 3 k v^2), B = 0.5 v q D:

    dA = 0.5 (dT + e (1 + t))      dq = 2 |t| dT + e t^2 + e q
    dD = 9 e c0 k v^2 + 2 e D      (3 k folded to a float: the third e)
    dG = e |grad| + dA + 2 e |B| + 0.5 |v| (dq D + q dD)
    dx:  |dy| dG + e |ref|

The 5 ulp are the OpenCL full-profile limit for tanh; no tighter figure is
documented for the device library.

RoPE: y1 = fma(x1, c, -fl(x2 s)) and its three siblings are two roundings each:
2 e (|x1 c| + |x2 s|) (2 e (|x1 s| + |x2 c|) for the second half), the
reference from the stored tables. inverse(forward(x)) is x (c^2 + s^2) for the
stored c, s; against x itself the bound is |x| |c^2 + s^2 - 1| plus the forward
bound carried through |c| and |s| plus the inverse's own bound.

colsum: depth e sum_r |x[r, c]|, depth the longest chain of roundings one
output sees: (trips - 1) per-thread additions (the first lands on 0), the LDS
combine of 32 lanes (31 roundings; 3 for the 4 lanes of the scalar kernel) and
gridDim.y - 1 atomics, all from ``launch_colsum``'s arithmetic restated in
``colsum_geometry``. mse_fwd sums non-negative terms, so its bound is relative:
(chain + 2) e for d^2 (x - y rounds once, squared) and a thread's chain of
fma, 10 e the block reduce (6 shuffle steps and 4 waves), (grid - 1) e the
atomics, 3 e for float(n), 1 / n and the last multiply. The two large colsum
cases (values in {-1, 0, 1}) and the large MSE case (x, y in {0, 1}) have only
exact partial sums and are asserted exactly: a summation bound at that size
would hide a dropped row.

Shapes. Flat ops, V = 8 (bf16) or 4 (fp32) elements per 16-byte vector:
n in {0, 1, V - 1, V, V + 1, 255 V + 3, 256 V + 1, 4 194 333}; the last is
2048 * 256 * 8 + 8 * 3 + 5: kMaxGrid blocks of 256 threads make a second trip
of three bf16 vectors (a third trip in fp32) and leave a tail. RoPE:
(1, 1, 1, 2), (3, 5, 7, 10) (all different and D / 2 odd, so a swapped decode
shows), (2, 3, 1, 6), (1, 4, 2, 128) with a 9-row table, (2, 1025, 4, 128)
with 512 pairs on a second trip. colsum: see COLSUM_SHAPES. The in-place and
out-parameter ops run on slices at an element offset of 8 inside NaN-filled
parents, as data_plane.py calls them; the canaries must survive.

NaN locality: one NaN input, once in the vector body and once in the tail,
comes out as NaN at that element alone (RoPE: its pair; colsum: its column;
MSE forward: the loss); everything else still meets its bound. ``relu_fwd`` of
NaN is not asserted (fmaxf gives 0, as BatchNorm's fused ReLU does), so for
add_relu only the other elements are checked.

The unmarked tests emulate each kernel family in fp32 on the CPU on the same
inputs: vector body and tail, the capped grid with its stride, RoPE's index
decode, both colsum geometries, the 64 x 64 transpose tile walk, the integer
bf16 rounding. Honest arithmetic stays at or below 1.0; every single defect in
MUTANTS exceeds 4x on a case that reaches it, or fails the equality of an exact
op. The CPU fallbacks of functional.py are held to the same bounds. Nothing
here was fitted to a result; the figures measured on an MI355X and by the
emulation are in csrc/README.md."""

import functools
import zlib

import numpy as np
import pytest
import torch

from baton_amd.ops import functional as BF

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
F64 = torch.float64
DTYPES = (BF16, FP32)
E = 2.0 ** -24
U = 2.0 ** -8
F = 1.0 + U
TINY = 2.0 ** -126
KBLOCK, KMAXGRID = 256, 2048
BIG = KMAXGRID * KBLOCK * 8 + 8 * 3 + 5
C0 = float(np.float32(0.7978845608))
K = float(np.float32(0.044715))
ALPHA = 0.3
DOUT = 1.7
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


def dn(dt):
    return "bf16" if dt == BF16 else "fp32"


def vec(dt):
    return 8 if dt == BF16 else 4


def store(dt):
    return U if dt == BF16 else 0.0


def flat_sizes(dt):
    v = vec(dt)
    return [1, v - 1, v, v + 1, 255 * v + 3, 256 * v + 1, BIG]


def lim(dt, ref, term):
    return store(dt) * ref.abs() + F * term


def worst(got, ref, bound):
    """max error / bound over the elements whose reference is not NaN. A NaN
    or inf that the reference does not have, a missing NaN, or an error where
    the bound is 0 counts as infinite."""
    if ref.numel() == 0:
        return 0.0 if got.numel() == 0 else float("inf")
    got = got.double().reshape(ref.shape)
    nan_ref = ref.isnan()
    if not torch.equal(got.isnan(), nan_ref):
        return float("inf")
    err = (got - ref).abs()
    inf, zero = torch.full_like(err, float("inf")), torch.zeros_like(err)
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, inf, zero))
    r = torch.where(torch.isfinite(got), r, inf)
    r = torch.where(nan_ref, zero, r)
    return r.max().item()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == FP32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(bits(a), bits(b))


# ---- fp32 arithmetic of the kernels on the CPU -----------------------------

def fma32(a, b, c):
    """fmaf: the product of two fp32 is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def rne_bf16(t32, trunc=False, keep_nan=False):
    """VecTraits<bf16>::from_float in integers: u + 0x7fff + lsb, upper half.
    keep_nan is cast_copy's own convert."""
    u = t32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if trunc:
        r = u >> 16
    else:
        r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16
    if keep_nan:
        r = torch.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, r)
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(BF16)


def store_emu(t32, dt, defect=None):
    if dt == FP32:
        return t32.float()
    return rne_bf16(t32.float(), trunc=(defect == "trunc_store"))


def stream_grid(n, gdiv):
    """elementwise_grid(n / gdiv + 1) of common.h."""
    b = (n // gdiv + 1 + KBLOCK - 1) // KBLOCK
    return max(1, min(b, KMAXGRID))


def cover(n, V, gdiv, defect=None):
    """Which elements a streaming kernel writes: thread t of grid * 256 takes
    vectors t, t + threads, ... and then the tail elements the same way."""
    done = torch.zeros(n, dtype=torch.bool)
    threads = stream_grid(n, gdiv) * KBLOCK
    nvec = n // V
    stop = nvec - 1 if defect == "drop_last_vector" else nvec
    t = torch.arange(threads)
    trip = 0
    while trip * threads < stop:
        i = t + trip * threads
        i = i[i < stop]
        done.view(-1)[: nvec * V].view(nvec, V)[i] = True
        trip += 1
        if defect == "no_second_trip":
            break
    if defect != "skip_tail":
        i = nvec * V + t
        done[i[i < n]] = True
    return done


# ---- the flat ops ----------------------------------------------------------

def gelu_parts(v):
    """float64 pieces of the tanh GELU with the kernel's float constants;
    1 + t and 1 - t^2 without their cancellation."""
    inner = C0 * (v + K * v ** 3)
    ex = torch.exp(-2 * inner.abs())
    onept = torch.where(inner >= 0, 2 / (1 + ex), 2 * ex / (1 + ex))
    t = torch.tanh(inner)
    q = 4 * ex / (1 + ex) ** 2
    dI = 2 * E * C0 * K * v.abs() ** 3 + 2 * E * inner.abs()
    dT = q * dI + 10 * E * t.abs()
    return onept, t, q, dT


def ref_gelu_fwd(i, dt):
    v = i["x"].double()
    onept, t, q, dT = gelu_parts(v)
    ref = 0.5 * v * onept
    return [(ref, lim(dt, ref, 0.5 * v.abs() * (dT + E * onept) + E * ref.abs()))]


def ref_gelu_bwd(i, dt):
    v, dy = i["x"].double(), i["dy"].double()
    onept, t, q, dT = gelu_parts(v)
    D = C0 * (1 + 3 * K * v * v)
    A = 0.5 * onept
    B = 0.5 * v * q * D
    grad = A + B
    dA = 0.5 * (dT + E * onept)
    dq = 2 * t.abs() * dT + E * t * t + E * q
    dD = 9 * E * C0 * K * v * v + 2 * E * D
    dG = E * grad.abs() + dA + 2 * E * B.abs() + 0.5 * v.abs() * (dq * D + q * dD)
    ref = dy * grad
    return [(ref, lim(dt, ref, dy.abs() * dG + E * ref.abs()))]


def emu_gelu_inner(v, defect):
    k = 0.0447 if defect == "gelu_k" else 0.044715
    return 0.7978845608 * fma32((k * v) * v, v, v), k


def emu_gelu_fwd(i, defect=None):
    v = i["x"].float()
    inner, _ = emu_gelu_inner(v, defect)
    return [(0.5 * v) * (1.0 + torch.tanh(inner))]


def emu_gelu_bwd(i, defect=None):
    v, dy = i["x"].float(), i["dy"].float()
    inner, k = emu_gelu_inner(v, defect)
    t = torch.tanh(inner)
    k3 = float(np.float32(3.0) * np.float32(k))
    dinner = 0.7978845608 * fma32(k3 * v, v, torch.ones_like(v))
    b = (0.5 * v) * (1.0 - t * t)
    if defect != "gelu_no_dinner":
        b = b * dinner
    return [dy * (0.5 * (1.0 + t) + b)]


def silu_parts(a):
    ex = torch.exp(-a.abs())
    sig = torch.where(a >= 0, 1 / (1 + ex), ex / (1 + ex))
    om = torch.where(a >= 0, ex / (1 + ex), 1 / (1 + ex))
    dsig = (om * (2 * a.abs() + 2) + 3) * E
    return sig, om, dsig


def ref_silu_fwd(i, dt):
    a, b = i["a"].double(), i["b"].double()
    sig, om, dsig = silu_parts(a)
    ref = a * sig * b
    return [(ref, lim(dt, ref, ref.abs() * (dsig + 2 * E)
                      + TINY * ((a * b).abs() + 1)))]


def ref_silu_bwd(i, dt):
    a, b, dy = i["a"].double(), i["b"].double(), i["dy"].double()
    sig, om, dsig = silu_parts(a)
    g = 1 + a * om
    da = dy * b * sig * g
    db = dy * a * sig
    w = (dy * b).abs()
    t_da = (w * (sig * dsig * (g.abs() + a.abs() * sig) + E * sig * a.abs() * om
                 + 2 * E * sig * g.abs()) + 2 * E * da.abs()
            + TINY * (w * (1 + a.abs()) + 1))
    t_db = db.abs() * (dsig + 2 * E) + TINY * ((dy * a).abs() + 1)
    return [(da, lim(dt, da, t_da)), (db, lim(dt, db, t_db))]


def emu_sig(a):
    return 1.0 / (1.0 + torch.exp(-a))


def emu_silu_fwd(i, defect=None):
    a, b = i["a"].float(), i["b"].float()
    return [(a * emu_sig(a)) * b]


def emu_silu_bwd(i, defect=None):
    a, b, dy = i["a"].float(), i["b"].float(), i["dy"].float()
    sig = emu_sig(a)
    dsilu = sig * fma32(a, 1.0 - sig, torch.ones_like(a))
    if defect == "silu_no_a_term":
        dsilu = sig
    silu = sig if defect == "silu_db_sig" else a * sig
    return [(dy * b) * dsilu, dy * silu]


def ref_add_relu(i, dt):
    s = i["a"].double() + i["b"].double()
    ref = s.clamp_min(0)
    ref = torch.where(s.isnan(), s, ref)
    return [(ref, lim(dt, ref, E * s.abs()))]


def ref_add_scaled(i, dt):
    ref = i["a"].double() + f32(ALPHA) * i["b"].double()
    return [(ref, lim(dt, ref, E * ref.abs()))]


def ref_scale(i, dt):
    ref = f32(ALPHA) * i["x"].double()
    return [(ref, lim(dt, ref, E * ref.abs()))]


def ref_mse_bwd(i, dt):
    x, y = i["x"].double(), i["y"].double()
    ref = 2 * f32(DOUT) / x.numel() * (x - y)
    return [(ref, lim(dt, ref, 3 * E * ref.abs()))]


def emu_add_relu(i, defect=None):
    s = i["a"].float() + i["b"].float()
    return [torch.where(s.isnan(), s, s.clamp_min(0))]


def emu_add_scaled(i, defect=None):
    al = 1.0 if defect == "ignore_alpha" else ALPHA
    a, b = i["a"].float(), i["b"].float()
    return [fma32(torch.full_like(b, al), b, a)]


def emu_scale(i, defect=None):
    return [ALPHA * i["x"].float()]


def emu_mse_bwd(i, defect=None):
    x, y = i["x"].float(), i["y"].float()
    n = x.numel() // vec(i["x"].dtype) if defect == "mse_n_over_v" else x.numel()
    c = np.float32(2.0) * np.float32(DOUT) / np.float32(max(n, 1))
    return [float(c) * (x - y)]


def sp(vals):
    return [s * v for v in vals for s in (1.0, -1.0)]


SP_SILU = sp((0.0, 2.0 ** -20, 1.0, 8.0, 20.0, 80.0, 100.0))
SP_GELU = sp((0.0, 2.0 ** -20, 0.5, 1.0, 3.0, 5.0, 8.0, 30.0))


def _dout():
    return torch.tensor(DOUT, dtype=FP32)


# name: inputs (name, std, specials), grid divisor, reference, emulation, GPU
# call, CPU fallback, outputs, the input that takes the NaN
SPEC = {
    "add_relu": dict(
        ins=[("a", 2.0, None), ("b", 2.0, None)], gdiv=8, ref=ref_add_relu,
        emu=emu_add_relu, gpu=lambda a, b: [OPS.add_relu_fwd(a, b)],
        cpu=lambda a, b: [BF.add_relu(a, b)], outs=["y"], nan="a"),
    "add_scaled": dict(
        ins=[("a", 2.0, None), ("b", 2.0, None)], gdiv=8, ref=ref_add_scaled,
        emu=emu_add_scaled, gpu=lambda a, b: [OPS.add_scaled_fwd(a, b, ALPHA)],
        cpu=lambda a, b: [BF.add_scaled(a, b, ALPHA)], outs=["z"], nan="b"),
    "scale": dict(
        ins=[("x", 2.0, None)], gdiv=8, ref=ref_scale, emu=emu_scale,
        gpu=lambda x: [OPS.scale_fwd(x, ALPHA)], cpu=None, outs=["z"], nan="x"),
    "gelu_fwd": dict(
        ins=[("x", 2.0, SP_GELU)], gdiv=4, ref=ref_gelu_fwd, emu=emu_gelu_fwd,
        gpu=lambda x: [OPS.gelu_fwd(x)], cpu=lambda x: [BF.gelu(x)],
        outs=["y"], nan="x"),
    "gelu_bwd": dict(
        ins=[("dy", 1.0, None), ("x", 2.0, SP_GELU)], gdiv=4, ref=ref_gelu_bwd,
        emu=emu_gelu_bwd, gpu=lambda dy, x: [OPS.gelu_bwd(dy, x)],
        cpu=lambda dy, x: [_grads(BF.gelu, [x], dy)[0]], outs=["dx"], nan="x"),
    "silu_fwd": dict(
        ins=[("a", 3.0, SP_SILU), ("b", 1.0, None)], gdiv=4, ref=ref_silu_fwd,
        emu=emu_silu_fwd, gpu=lambda a, b: [OPS.silu_mul_fwd(a, b)],
        cpu=lambda a, b: [BF.silu_mul(a, b)], outs=["y"], nan="a"),
    "silu_bwd": dict(
        ins=[("dy", 1.0, None), ("a", 3.0, SP_SILU), ("b", 1.0, None)], gdiv=4,
        ref=ref_silu_bwd, emu=emu_silu_bwd,
        gpu=lambda dy, a, b: OPS.silu_mul_bwd(dy, a, b),
        cpu=lambda dy, a, b: _grads(BF.silu_mul, [a, b], dy),
        outs=["da", "db"], nan="a"),
    "mse_bwd": dict(
        ins=[("x", 1.0, None), ("y", 1.0, None)], gdiv=8, ref=ref_mse_bwd,
        emu=emu_mse_bwd,
        gpu=lambda x, y: [OPS.mse_bwd(x, y, _dout().to(x.device))],
        cpu=lambda x, y: [_grads(BF.mse_loss, [x, y], _dout())[0]],
        outs=["dx"], nan="x"),
}
FLAT_CASES = [(op, dt) for op in SPEC for dt in DTYPES]


def flat_id(c):
    return f"{c[0]}_{dn(c[1])}"


def _grads(fn, ins, dy):
    """Gradients of a functional.py op through its own backward."""
    leaves = [t.clone().requires_grad_(True) for t in ins]
    fn(*leaves).backward(dy)
    return [t.grad if t.grad is not None else torch.zeros_like(t)
            for t in leaves]


def make_inputs(op, n, dt):
    out = {}
    for name, std, special in SPEC[op]["ins"]:
        seed = zlib.crc32(f"{op}/{name}/{n}".encode())
        g = torch.Generator().manual_seed(seed)
        t = torch.randn(n, generator=g).mul(std)
        if special:
            s = torch.tensor(special)
            k = min(n, len(s))
            t[:k] = s[:k]
            if n >= 2 * len(s):     # and in the last vector / the tail
                t[n - len(s):] = s
        out[name] = t.to(dt)
    return out


@functools.lru_cache(maxsize=None)
def flat_case(op, n, dt):
    """Stored inputs and [(float64 reference, bound)] per output; shared by
    the GPU, emulation and fallback tests and never modified."""
    ins = make_inputs(op, n, dt)
    return ins, SPEC[op]["ref"](ins, dt)


def emu_ratio(op, n, dt, defect=None):
    ins, refs = flat_case(op, n, dt)
    outs = SPEC[op]["emu"](ins, defect)
    done = cover(n, vec(dt), SPEC[op]["gdiv"], defect)
    worst_r = 0.0
    for o, (ref, bound) in zip(outs, refs):
        o = store_emu(o, dt, defect)
        o = torch.where(done, o, torch.full_like(o, NAN))   # never written
        worst_r = max(worst_r, worst(o, ref, bound))
    return worst_r


# (defect, op, dtype, n): a case that reaches the defect
V8, V4 = 8, 4
MUTANTS = [
    ("skip_tail", "scale", BF16, V8 + 1),
    ("skip_tail", "silu_bwd", FP32, 255 * V4 + 3),
    ("drop_last_vector", "add_relu", BF16, 256 * V8 + 1),
    ("drop_last_vector", "gelu_fwd", FP32, V4),
    ("no_second_trip", "scale", BF16, BIG),
    ("no_second_trip", "scale", FP32, BIG),
    ("silu_no_a_term", "silu_bwd", FP32, 256 * V4 + 1),
    ("silu_no_a_term", "silu_bwd", BF16, 256 * V8 + 1),
    ("silu_db_sig", "silu_bwd", FP32, 256 * V4 + 1),
    ("silu_db_sig", "silu_bwd", BF16, 256 * V8 + 1),
    ("gelu_k", "gelu_fwd", FP32, 256 * V4 + 1),
    ("gelu_k", "gelu_bwd", FP32, 256 * V4 + 1),
    ("gelu_no_dinner", "gelu_bwd", FP32, 256 * V4 + 1),
    ("gelu_no_dinner", "gelu_bwd", BF16, 256 * V8 + 1),
    ("ignore_alpha", "add_scaled", FP32, 255 * V4 + 3),
    ("ignore_alpha", "add_scaled", BF16, 255 * V8 + 3),
    ("mse_n_over_v", "mse_bwd", FP32, 255 * V4 + 3),
    ("mse_n_over_v", "mse_bwd", BF16, 255 * V8 + 3),
]


@pytest.mark.parametrize("case", FLAT_CASES, ids=flat_id)
def test_flat_emulation_honest(case):
    op, dt = case
    sizes = [n for n in flat_sizes(dt) if n != BIG or op in ("scale", "silu_fwd")]
    for n in sizes:
        r = emu_ratio(op, n, dt)
        print(f"emu {op} {dn(dt)} n={n}: {r:.3f}")
        assert r <= 1.0, (op, dn(dt), n, r)


@pytest.mark.parametrize(
    "m", MUTANTS, ids=lambda m: f"{m[0]}-{m[1]}_{dn(m[2])}_{m[3]}")
def test_flat_emulation_mutants(m):
    defect, op, dt, n = m
    r = emu_ratio(op, n, dt, defect)
    print(f"mutant {defect} {op} {dn(dt)} n={n}: {r:.3g}")
    assert r >= 4.0, (m, r)


@pytest.mark.parametrize("case", [c for c in FLAT_CASES if SPEC[c[0]]["cpu"]],
                         ids=flat_id)
def test_flat_cpu_fallback(case):
    op, dt = case
    for n in flat_sizes(dt)[:-1]:
        ins, refs = flat_case(op, n, dt)
        outs = SPEC[op]["cpu"](*[t.clone() for t in ins.values()])
        for name, o, (ref, bound) in zip(SPEC[op]["outs"], outs, refs):
            assert o.dtype == dt
            r = worst(o.detach(), ref, bound)
            print(f"cpu {op}.{name} {dn(dt)} n={n}: {r:.3f}")
            assert r <= 1.0, (op, name, dn(dt), n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FLAT_CASES, ids=flat_id)
def test_flat_gpu(case):
    op, dt = case
    top = {}
    for n in flat_sizes(dt):
        ins, refs = flat_case(op, n, dt)
        outs = SPEC[op]["gpu"](*[t.to(DEV) for t in ins.values()])
        for name, o, (ref, bound) in zip(SPEC[op]["outs"], outs, refs):
            assert o.dtype == dt and o.numel() == n
            r = worst(o.cpu(), ref, bound)
            top[name] = max(top.get(name, 0.0), r)
            assert r <= 1.0, (op, name, dn(dt), n, r)
    print(f"gpu {op} {dn(dt)}: " +
          ", ".join(f"{k} {v:.3f}" for k, v in top.items()))
    empty = [torch.empty(0, dtype=dt, device=DEV) for _ in SPEC[op]["ins"]]
    for o in SPEC[op]["gpu"](*empty):
        assert o.numel() == 0 and o.dtype == dt


def nan_case(op, dt, where):
    """3 vectors and a tail of V - 1; the NaN in vector 1 or at the last tail
    element. The reference is rebuilt from the poisoned inputs."""
    v = vec(dt)
    n = 4 * v - 1
    p = v + 1 if where == "body" else n - 1
    ins = {k: t.clone() for k, t in make_inputs(op, n, dt).items()}
    ins[SPEC[op]["nan"]][p] = NAN
    return ins, SPEC[op]["ref"](ins, dt), p, n


def check_nan_outs(op, dt, outs, refs, p, n):
    only_p = torch.zeros(n, dtype=torch.bool)
    only_p[p] = True
    for name, o, (ref, bound) in zip(SPEC[op]["outs"], outs, refs):
        o = o.detach().cpu()
        if op == "add_relu":        # relu(NaN) itself is not asserted
            keep = ~only_p
            o, ref, bound = o[keep], ref[keep], bound[keep]
            assert not o.isnan().any()
        else:
            assert torch.equal(ref.isnan(), only_p), (op, name)
            assert torch.equal(o.isnan(), only_p), (op, name, dn(dt))
        assert worst(o, ref, bound) <= 1.0, (op, name, dn(dt))


@pytest.mark.parametrize("where", ["body", "tail"])
@pytest.mark.parametrize("case", FLAT_CASES, ids=flat_id)
def test_flat_nan_locality_emulation(case, where):
    op, dt = case
    ins, refs, p, n = nan_case(op, dt, where)
    outs = [store_emu(o, dt) for o in SPEC[op]["emu"](ins)]
    check_nan_outs(op, dt, outs, refs, p, n)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["body", "tail"])
@pytest.mark.parametrize("case", FLAT_CASES, ids=flat_id)
def test_flat_nan_locality_gpu(case, where):
    op, dt = case
    ins, refs, p, n = nan_case(op, dt, where)
    outs = SPEC[op]["gpu"](*[t.to(DEV) for t in ins.values()])
    check_nan_outs(op, dt, outs, refs, p, n)


# ---- exact ops -------------------------------------------------------------

def relu_inputs(n, dt):
    g = torch.Generator().manual_seed(7919 + n)
    x = torch.randn(n, generator=g)
    x[::5] = 0.0
    x[1::7] = -0.0
    return x.to(dt)


def check_relu_fwd(x, y):
    pos = x > 0
    assert y.dtype == x.dtype and y.shape == x.shape
    assert torch.equal(bits(y)[pos], bits(x)[pos])
    assert bool((y[~pos] == 0).all())


def relu_bwd_inputs(n, dt):
    """dy is NaN on a third of the masked elements."""
    y = relu_inputs(n, dt)
    g = torch.Generator().manual_seed(104729 + n)
    dy = torch.randn(n, generator=g)
    dead = (~(y > 0)).nonzero().flatten()
    dy[dead[::3]] = NAN
    return dy.to(dt), y


def check_relu_bwd(dy, y, dx):
    pos = y > 0
    assert dx.dtype == dy.dtype and dx.shape == dy.shape
    assert torch.equal(bits(dx)[pos], bits(dy)[pos])
    assert bool((dx[~pos] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_relu_exact_gpu(dt):
    for n in [0] + flat_sizes(dt):
        x = relu_inputs(n, dt)
        check_relu_fwd(x, OPS.relu_fwd(x.to(DEV)).cpu())
        dy, y = relu_bwd_inputs(n, dt)
        check_relu_bwd(dy, y, OPS.relu_bwd(dy.to(DEV), y.to(DEV)).cpu())


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_relu_exact_cpu_fallback(dt):
    for n in [0] + flat_sizes(dt)[:-1]:
        x = relu_inputs(n, dt)
        check_relu_fwd(x, BF.relu(x))
        dy, y = relu_bwd_inputs(n, dt)
        leaf = y.clone().requires_grad_(True)
        out = BF.relu(leaf)
        out.backward(dy)
        check_relu_bwd(dy, out.detach(), leaf.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_scale_pow2_exact_gpu(dt):
    for n in flat_sizes(dt):
        x = make_inputs("scale", n, dt)["x"]
        for alpha in (0.5, 4.0, -2.0):
            want = (x.float() * alpha).to(dt)       # exact
            assert same_bits(OPS.scale_fwd(x.to(DEV), alpha).cpu(), want)


def canaried(n, dt, off=8, pad=8):
    """A NaN-filled parent and its slice [off : off + n], as data_plane.py
    slices its flat buffers; off is a multiple of 8 elements."""
    parent = torch.full((off + n + pad,), NAN, dtype=dt, device=DEV)
    return parent, parent[off:off + n]


def canaries_intact(parent, n, off=8):
    return bool(parent[:off].isnan().all()) and bool(parent[off + n:].isnan().all())


def put(values):
    """values inside a canaried parent on the GPU."""
    parent, view = canaried(values.numel(), values.dtype)
    view.copy_(values)
    return parent, view


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_scale_cast_gpu(dt):
    """Power-of-two alpha and alpha 1 bit for bit, a general alpha to e |ref|,
    one NaN staying where it is; canaries on both sides untouched."""
    top = 0.0
    for n in [0] + flat_sizes(dt):
        x = make_inputs("scale", n, dt)["x"]
        v = vec(dt)
        for alpha, nan_at in ((1.0, None), (0.25, None), (ALPHA, None),
                              (ALPHA, v + 1), (ALPHA, n - 1)):
            src = x.clone()
            if nan_at is not None:
                if n < 2 * v + 2:
                    continue
                src[nan_at] = NAN
            sp_, sv = put(src)
            dp, dv = canaried(n, FP32)
            OPS.scale_cast(dv, sv, alpha)
            got = dv.cpu()
            assert canaries_intact(dp, n) and canaries_intact(sp_, n)
            assert same_bits(sv.cpu(), src)
            ref = f32(alpha) * src.double()
            if alpha != ALPHA:
                assert same_bits(got, ref.float())
            else:
                r = worst(got, ref, F * E * ref.abs())
                top = max(top, r)
                assert r <= 1.0, (dn(dt), n, alpha, nan_at, r)
    print(f"gpu scale_cast {dn(dt)}: {top:.3f}")


@pytest.mark.gpu
def test_axpby_gpu():
    top = 0.0
    a, b = 0.3, -1.7
    for n in [0] + flat_sizes(FP32):
        ins = make_inputs("add_scaled", n, FP32)
        for nan_in, nan_at in ((None, None), ("a", 5), ("b", n - 1)):
            x, y = ins["a"].clone(), ins["b"].clone()
            if nan_in:
                if n < 7:
                    continue
                (x if nan_in == "a" else y)[nan_at] = NAN
            xp, xv = put(x)
            yp, yv = put(y)
            OPS.axpby(yv, xv, a, b)
            assert canaries_intact(yp, n) and canaries_intact(xp, n)
            assert same_bits(xv.cpu(), x)
            by = f32(b) * y.double()
            ref = f32(a) * x.double() + by
            r = worst(yv.cpu(), ref, F * E * (by.abs() + ref.abs()))
            top = max(top, r)
            assert r <= 1.0, (n, nan_in, r)
    print(f"gpu axpby fp32: {top:.3f}")


def i32(*patterns):
    a = np.array(patterns, dtype=np.uint32).view(np.int32)
    return torch.from_numpy(a.copy()).view(FP32)


# fp32 bit patterns for cast_copy<bf16>
CAST_TABLE = i32(
    0x00000000, 0x80000000,                 # +-0
    0x00000001, 0x80000001,                 # smallest subnormals
    0x007FFFFF, 0x807FFFFF,                 # largest subnormals
    0x3F808000, 0xBF808000,                 # tie, down to even 0x3f80
    0x3F818000, 0xBF818000,                 # tie, up to even 0x3f82
    0x3F807FFF, 0x3F808001,                 # just under / over a tie
    0x7F7F7FFF, 0xFF7F7FFF,                 # largest below the overflow tie
    0x7F7F8000, 0xFF7F8000,                 # the overflow tie: inf
    0x7F800000, 0xFF800000,                 # +-inf
    0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001, 0xFF800001,   # NaNs that the shared
    0x7FC00000, 0xFFC00000, 0x7F80FFFF)     # converter loses, and safe ones
CAST_NAN = CAST_TABLE.isnan()


def check_cast_bf16(got, src):
    want = src.to(BF16)                     # torch's CPU conversion
    nan = src.isnan()
    assert got.dtype == BF16
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(bits(got)[~nan], bits(want)[~nan])


def test_bf16_rounding_emulation():
    """The integer rounding against torch's CPU conversion; what the shared
    converter does to three NaN patterns; cast_copy's own convert keeps them;
    a truncating store fails the equality."""
    ok = ~CAST_NAN
    assert torch.equal(bits(rne_bf16(CAST_TABLE))[ok],
                       bits(CAST_TABLE.to(BF16))[ok])
    lost = bits(rne_bf16(i32(0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001))).tolist()
    assert [v & 0xFFFF for v in lost] == [0x8000, 0x0000, 0x7F80]
    assert bool(rne_bf16(i32(0x7FC00000, 0xFFC00000, 0x7FFF0000)).isnan().all())
    check_cast_bf16(rne_bf16(CAST_TABLE, keep_nan=True), CAST_TABLE)
    with pytest.raises(AssertionError):
        check_cast_bf16(rne_bf16(CAST_TABLE, trunc=True, keep_nan=True),
                        CAST_TABLE)
    x = make_inputs("scale", 255 * 8 + 3, FP32)["x"]
    assert same_bits(rne_bf16(x), x.to(BF16))
    assert not same_bits(rne_bf16(x, trunc=True), x.to(BF16))


@pytest.mark.gpu
def test_cast_copy_bf16_special_values_gpu():
    T = CAST_TABLE.numel()
    layouts = [(8 * 4, 0)]                  # the table in the vector body
    layouts += [(8 + 7, k) for k in range(0, T, 7)]   # 7 of it in the tail
    for n, k in layouts:
        src = torch.ones(max(n, T), dtype=FP32)
        if k == 0 and n >= T:
            src[:T] = CAST_TABLE
        else:
            src = src[:n]
            part = CAST_TABLE[k:k + 7]
            src[8:8 + part.numel()] = part
        n = src.numel()
        sp_, sv = put(src)
        dp, dv = canaried(n, BF16)
        OPS.cast_copy(dv, sv)
        assert canaries_intact(dp, n) and canaries_intact(sp_, n)
        check_cast_bf16(dv.cpu(), src)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_cast_copy_gpu(dt):
    """fp32 -> fp32 is a copy, fp32 -> bf16 is torch's rounding, at every
    flat size, inside canaried parents."""
    for n in [0] + flat_sizes(dt):
        src = make_inputs("scale", n, FP32)["x"]
        sp_, sv = put(src)
        dp, dv = canaried(n, dt)
        OPS.cast_copy(dv, sv)
        assert canaries_intact(dp, n) and canaries_intact(sp_, n)
        assert same_bits(sv.cpu(), src)
        assert same_bits(dv.cpu(), src.to(dt))


# ---- transpose -------------------------------------------------------------

TRANSPOSE_SHAPES = [(1, 1), (64, 64), (63, 65), (65, 63), (7, 200), (130, 9),
                    (129, 8), (130, 200)]


def distinct(R, C, dt):
    """Every element different, so a misplaced one cannot cancel."""
    if dt == FP32:
        return torch.arange(R * C, dtype=FP32).reshape(R, C)
    assert R * C < 2 ** 15
    return torch.arange(R * C, dtype=torch.int16).view(BF16).reshape(R, C)


def emu_transpose(x, defect=None):
    """transpose_kernel's tile walk: 256 threads, 16-byte runs, the scalar
    load where a run crosses C and the partial store where one crosses R."""
    R, C = x.shape
    EL = 16 // x.element_size()
    TPR = 64 // EL
    src = bits(x).reshape(-1)
    out = torch.full((C * R,), -1, dtype=src.dtype)
    for by in range((R + 63) // 64):
        for bx in range((C + 63) // 64):
            r0, c0 = by * 64, bx * 64
            tile = torch.zeros(64, 64 + EL, dtype=src.dtype)
            for idx in range(64 * TPR):
                r, cc = idx // TPR, (idx % TPR) * EL
                if r0 + r < R and c0 + cc + EL <= C:
                    o = (r0 + r) * C + c0 + cc
                    tile[r, cc:cc + EL] = src[o:o + EL]
                elif defect != "transpose_zero_fill":
                    for j in range(EL):
                        if r0 + r < R and c0 + cc + j < C:
                            tile[r, cc + j] = src[(r0 + r) * C + c0 + cc + j]
            for idx in range(64 * TPR):
                c, rr = idx // TPR, (idx % TPR) * EL
                if c0 + c >= C:
                    continue
                v = tile[rr:rr + EL, c]
                o = (c0 + c) * R + r0 + rr
                if r0 + rr + EL <= R:
                    out[o:o + EL] = v
                else:
                    for j in range(EL):
                        if r0 + rr + j < R:
                            out[o + j] = v[j]
    return out.view(x.dtype).reshape(C, R)


def transpose_paths(R, C, dt):
    """(scalar load taken, partial store taken) for a shape."""
    EL = 4 if dt == FP32 else 8
    return C % EL != 0, R % EL != 0


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_transpose_emulation(dt):
    hit = [False, False]
    for R, C in TRANSPOSE_SHAPES:
        if (R, C) == (130, 200):
            continue                # the same walk twelve times: slow here
        x = distinct(R, C, dt)
        assert same_bits(emu_transpose(x), x.t().contiguous()), (R, C)
        a, b = transpose_paths(R, C, dt)
        hit = [hit[0] or a, hit[1] or b]
    assert hit == [True, True]
    x = distinct(63, 65, dt)
    assert not same_bits(emu_transpose(x, "transpose_zero_fill"),
                         x.t().contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_transpose2d_gpu(dt):
    hit = [False, False]
    for R, C in TRANSPOSE_SHAPES:
        x = distinct(R, C, dt)
        got = OPS.transpose2d(x.to(DEV)).cpu()
        assert got.shape == (C, R)
        assert same_bits(got, x.t().contiguous()), (R, C, dn(dt))
        a, b = transpose_paths(R, C, dt)
        hit = [hit[0] or a, hit[1] or b]
    assert hit == [True, True]
    assert OPS.transpose2d(torch.empty(0, 5, dtype=dt, device=DEV)).shape == (5, 0)


# ---- RoPE ------------------------------------------------------------------

# (B, S, H, D, table rows)
ROPE_SHAPES = [(1, 1, 1, 2, 1), (3, 5, 7, 10, 5), (2, 3, 1, 6, 3),
               (1, 4, 2, 128, 4), (1, 4, 2, 128, 9), (2, 1025, 4, 128, 1025)]


def rope_id(c):
    return "x".join(str(v) for v in c[:4]) + f"_rows{c[4]}"


@functools.lru_cache(maxsize=None)
def rope_case(shape, dt):
    B, S, H, D, rows = shape
    n = B * S * H * D
    g = torch.Generator().manual_seed(15485863 + n + rows)
    x = torch.randn(n, generator=g) + torch.arange(n) % 251 / 16.0
    x = x.reshape(B, S, H, D).to(dt)
    cos_t, sin_t = BF.rope_tables(rows, D)
    if rows > S:                    # the rows past S must never be read
        cos_t[S:] = NAN
        sin_t[S:] = NAN
    return x, cos_t.contiguous(), sin_t.contiguous()


def rope_ref(x, cos_t, sin_t, dt, inverse):
    """float64 from the stored tables, and the bound."""
    S, half = x.shape[1], x.shape[3] // 2
    xd = x.double()
    x1, x2 = xd[..., :half], xd[..., half:]
    c = cos_t[:S].double()[None, :, None, :]
    s = sin_t[:S].double()[None, :, None, :]
    if inverse:
        s = -s
    ref = torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                     (x1 * s).abs() + (x2 * c).abs()], dim=-1)
    return ref, lim(dt, ref, 2 * E * mag)


def rope_roundtrip_bound(x, cos_t, sin_t, dt):
    """inverse(forward(x)) against x: x (c^2 + s^2 - 1), the forward bound
    through |c| and |s|, and the inverse's own bound on the forward result."""
    S, half = x.shape[1], x.shape[3] // 2
    c = cos_t[:S].double()[None, :, None, :].abs()
    s = sin_t[:S].double()[None, :, None, :].abs()
    y, by = rope_ref(x, cos_t, sin_t, dt, False)
    _, bz = rope_ref(y, cos_t, sin_t, dt, True)
    b1, b2 = by[..., :half], by[..., half:]
    carried = torch.cat([c * b1 + s * b2, s * b1 + c * b2], dim=-1)
    off = (c * c + s * s - 1).abs()
    return torch.cat([off, off], dim=-1) * x.double().abs() + carried + bz


def emu_rope(x, cos_t, sin_t, inverse, defect=None):
    """rope_kernel's decode of the flat pair index, on flat arrays."""
    B, S, H, D = x.shape
    dt = x.dtype
    half = D // 2
    if defect == "rope_half_up":
        half += half % 2
    total = x.numel() // 2
    xf = x.float().reshape(-1)
    cf, sf = cos_t.reshape(-1), sin_t.reshape(-1)
    y = torch.full((x.numel(),), NAN)
    grid = max(1, min((total + KBLOCK - 1) // KBLOCK, KMAXGRID))
    i = torch.arange(total)
    if defect == "no_second_trip":
        i = i[: grid * KBLOCK]
    d = i % half
    t = i // half
    h = t % H
    t2 = t // H
    s = t2 % S
    b = t2 // S
    if defect == "rope_swap_hs":    # the address of a [B, H, S, D] layout
        base = ((b * H + h) * S + s) * D + d
    else:
        base = ((b * S + s) * H + h) * D + d
    row = b * S + s if defect == "rope_row_bs" else s
    ti = row * half + d
    ok = base + half < x.numel()
    base, ti = base[ok], ti[ok]
    pad = torch.full((int(ti.max()) + 1 - cf.numel(),), NAN) \
        if int(ti.max()) >= cf.numel() else cf[:0]     # past the table
    c, sn = torch.cat([cf, pad])[ti], torch.cat([sf, pad])[ti]
    x1, x2 = xf[base], xf[base + half]
    if inverse:
        y1 = fma32(x1, c, x2 * sn)
        y2 = fma32(x2, c, -x1 * sn)
    else:
        y1 = fma32(x1, c, -x2 * sn)
        y2 = fma32(x1, -sn if defect == "rope_sign" else sn, x2 * c)
    y[base] = y1
    y[base + half] = y2
    return store_emu(y, dt).reshape(x.shape)


ROPE_MUTANTS = [
    ("rope_sign", (3, 5, 7, 10, 5)), ("rope_row_bs", (3, 5, 7, 10, 5)),
    ("rope_swap_hs", (3, 5, 7, 10, 5)), ("rope_half_up", (3, 5, 7, 10, 5)),
    ("rope_half_up", (2, 3, 1, 6, 3)),
    ("no_second_trip", (2, 1025, 4, 128, 1025)),
]


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=rope_id)
def test_rope_emulation(shape, dt):
    x, cos_t, sin_t = rope_case(shape, dt)
    for inverse in (False, True):
        ref, bound = rope_ref(x, cos_t, sin_t, dt, inverse)
        r = worst(emu_rope(x, cos_t, sin_t, inverse), ref, bound)
        print(f"emu rope {rope_id(shape)} {dn(dt)} inv={inverse}: {r:.3f}")
        assert r <= 1.0
    if shape[4] == shape[1] and x.numel() < 10 ** 5:    # the CPU fallback
        ref, bound = rope_ref(x, cos_t, sin_t, dt, False)
        leaf = x.clone().requires_grad_(True)
        y = BF.rope(leaf, cos_t, sin_t)
        assert worst(y.detach(), ref, bound) <= 1.0
        y.backward(x)
        ref, bound = rope_ref(x, cos_t, sin_t, dt, True)
        assert worst(leaf.grad, ref, bound) <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
@pytest.mark.parametrize("m", ROPE_MUTANTS, ids=lambda m: f"{m[0]}-{rope_id(m[1])}")
def test_rope_mutants(m, dt):
    defect, shape = m
    x, cos_t, sin_t = rope_case(shape, dt)
    ref, bound = rope_ref(x, cos_t, sin_t, dt, False)
    r = worst(emu_rope(x, cos_t, sin_t, False, defect), ref, bound)
    print(f"mutant {defect} {rope_id(shape)} {dn(dt)}: {r:.3g}")
    assert r >= 4.0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=rope_id)
def test_rope_gpu(shape, dt):
    x, cos_t, sin_t = rope_case(shape, dt)
    xg, cg, sg = x.to(DEV), cos_t.to(DEV), sin_t.to(DEV)
    out = {}
    for inverse in (False, True):
        ref, bound = rope_ref(x, cos_t, sin_t, dt, inverse)
        got = OPS.rope(xg, cg, sg, inverse)
        assert got.dtype == dt and got.shape == x.shape
        out[inverse] = worst(got.cpu(), ref, bound)
    y = OPS.rope(xg, cg, sg, False)
    z = OPS.rope(y, cg, sg, True).cpu()
    rt = worst(z, x.double(), rope_roundtrip_bound(x, cos_t, sin_t, dt))
    print(f"gpu rope {rope_id(shape)} {dn(dt)}: fwd {out[False]:.3f} "
          f"inv {out[True]:.3f} roundtrip {rt:.3f}")
    assert out[False] <= 1.0 and out[True] <= 1.0 and rt <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_rope_nan_locality_gpu(dt):
    """A NaN comes out at its pair (d, d + D / 2) and nowhere else."""
    shape = (3, 5, 7, 10, 5)
    x0, cos_t, sin_t = rope_case(shape, dt)
    for pos in ((1, 2, 3, 1), (2, 4, 6, 9)):
        x = x0.clone()
        x[pos] = NAN
        want = torch.zeros(x.shape, dtype=torch.bool)
        want[pos] = True
        want[pos[:3] + ((pos[3] + 5) % 10,)] = True
        for inverse in (False, True):
            ref, bound = rope_ref(x, cos_t, sin_t, dt, inverse)
            assert torch.equal(ref.isnan(), want)
            got = OPS.rope(x.to(DEV), cos_t.to(DEV), sin_t.to(DEV), inverse)
            assert worst(got.cpu(), ref, bound) <= 1.0


# ---- colsum ----------------------------------------------------------------

COLSUM_SHAPES = [
    (1, 64),        # vector kernel, one row
    (33, 128),      # a 33rd row: lane 0 again
    (129, 64),      # gridDim.y = 2, the second block has one row
    (128, 192),     # three channel blocks
    (5, 1), (4, 63), (130, 65), (257, 100),     # scalar kernel (C % 64 != 0)
    (3, 65600),     # 1025 channel blocks clamp target to 1
]
COLSUM_EXACT = [(131200, 64), (131200, 8)]      # rows_per_block = 129 > 128


def colsum_geometry(R, C):
    """launch_colsum's arithmetic: (vector kernel, row lanes, rows per block,
    gridDim.y, depth of the longest rounding chain of one output)."""
    cgrid = (C + 63) // 64
    target = max(1, 1024 // max(cgrid, 1))
    rpb = max(128, (R + target - 1) // target)
    gy = (R + rpb - 1) // rpb
    vecp = C % 64 == 0
    lanes = 32 if vecp else 4
    trips = (min(rpb, R) + lanes - 1) // lanes
    return vecp, lanes, rpb, gy, (trips - 1) + (lanes - 1) + (gy - 1)


def test_colsum_geometry():
    assert colsum_geometry(1, 64) == (True, 32, 128, 1, 31)
    assert colsum_geometry(129, 64) == (True, 32, 128, 2, 3 + 31 + 1)
    assert colsum_geometry(257, 100) == (False, 4, 128, 3, 31 + 3 + 2)
    assert colsum_geometry(3, 65600)[2:4] == (128, 1)
    assert colsum_geometry(131200, 64)[:4] == (True, 32, 129, 1018)
    assert colsum_geometry(131200, 8)[:4] == (False, 4, 129, 1018)


@functools.lru_cache(maxsize=None)
def colsum_case(R, C, dt):
    g = torch.Generator().manual_seed(32452843 + 1000 * R + C)
    if (R, C) in COLSUM_EXACT:
        x = torch.randint(-1, 2, (R, C), generator=g).to(dt)
        return x, x.double().sum(0), None
    x = (torch.randn(R, C, generator=g) * 2).to(dt)
    depth = colsum_geometry(R, C)[4]
    return x, x.double().sum(0), F * depth * E * x.double().abs().sum(0)


def emu_colsum(x, defect=None):
    R, C = x.shape
    vecp, lanes, rpb, gy, _ = colsum_geometry(R, C)
    xf = x.float()
    if defect == "colsum_drop_channel" and not vecp:
        xf = xf.clone()
        xf[:, C - 1] = 0.0
    pad = torch.zeros(gy * rpb, C)
    pad[:R] = xf
    trips = (rpb + lanes - 1) // lanes
    blk = torch.zeros(gy, trips * lanes, C)
    blk[:, :rpb] = pad.reshape(gy, rpb, C)
    blk = blk.reshape(gy, trips, lanes, C)
    acc = torch.zeros(gy, lanes, C)
    for t in range(trips):
        acc = acc + blk[:, t]
    if defect == "colsum_drop_lane":
        acc[:, lanes - 1] = 0.0
    if vecp:
        tot = torch.zeros(gy, C)
        for lane in range(lanes):
            tot = tot + acc[:, lane]
    else:
        tot = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    out = torch.zeros(C)
    for by in range(gy - 1 if defect == "colsum_drop_block" else gy):
        out = out + tot[by]
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_colsum_emulation(dt):
    for R, C in COLSUM_SHAPES:
        x, ref, bound = colsum_case(R, C, dt)
        r = worst(emu_colsum(x), ref, bound)
        print(f"emu colsum {R}x{C} {dn(dt)}: {r:.3f}")
        assert r <= 1.0, (R, C, r)
    for R, C in COLSUM_EXACT[1:] if dt == FP32 else COLSUM_EXACT:
        x, ref, _ = colsum_case(R, C, dt)
        assert torch.equal(emu_colsum(x).double(), ref)
    for defect, shapes in (("colsum_drop_lane", [(257, 100), (33, 128)]),
                           ("colsum_drop_block", [(129, 64), (130, 65)]),
                           ("colsum_drop_channel", [(4, 63), (130, 65)])):
        for R, C in shapes:
            x, ref, bound = colsum_case(R, C, dt)
            r = worst(emu_colsum(x, defect), ref, bound)
            print(f"mutant {defect} {R}x{C} {dn(dt)}: {r:.3g}")
            assert r >= 4.0, (defect, R, C, r)
    x, ref, _ = colsum_case(131200, 8, dt)
    assert not torch.equal(emu_colsum(x, "colsum_drop_block").double(), ref)
    assert not torch.equal(emu_colsum(x, "colsum_drop_lane").double(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_colsum_gpu(dt):
    top = 0.0
    for R, C in COLSUM_SHAPES:
        x, ref, bound = colsum_case(R, C, dt)
        got = OPS.colsum(x.to(DEV))
        assert got.dtype == FP32 and got.shape == (C,)
        r = worst(got.cpu(), ref, bound)
        top = max(top, r)
        assert r <= 1.0, (R, C, dn(dt), r)
    print(f"gpu colsum {dn(dt)}: {top:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
@pytest.mark.parametrize("shape", COLSUM_EXACT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colsum_large_exact_gpu(shape, dt):
    x, ref, _ = colsum_case(*shape, dt)
    assert torch.equal(OPS.colsum(x.to(DEV)).cpu().double(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_colsum_nan_locality_gpu(dt):
    for (R, C), (r, c) in (((129, 64), (128, 9)), ((130, 65), (77, 64))):
        x0, _, _ = colsum_case(R, C, dt)
        x = x0.clone()
        x[r, c] = NAN
        depth = colsum_geometry(R, C)[4]
        ref = x.double().sum(0)
        assert ref.isnan().nonzero().flatten().tolist() == [c]
        bound = F * depth * E * x.double().abs().sum(0)
        assert worst(OPS.colsum(x.to(DEV)).cpu(), ref, bound) <= 1.0


# ---- MSE forward -----------------------------------------------------------

def mse_geometry(n, dt):
    """(grid, roundings of the longest chain) of mse_fwd_kernel."""
    V = vec(dt)
    grid = stream_grid(n, 8)
    threads = grid * KBLOCK
    chain = V * ((n // V + threads - 1) // threads) + 1
    return grid, (chain + 2) + 10 + (grid - 1) + 3


@functools.lru_cache(maxsize=None)
def mse_case(n, dt):
    ins = make_inputs("mse_bwd", n, dt)
    x, y = ins["x"], ins["y"]
    ref = ((x.double() - y.double()) ** 2).sum() / n
    return x, y, ref.reshape(()), F * mse_geometry(n, dt)[1] * E * ref.reshape(())


@functools.lru_cache(maxsize=None)
def mse_binary_case(dt):
    g = torch.Generator().manual_seed(49979687)
    x = torch.randint(0, 2, (BIG,), generator=g).to(dt)
    y = torch.randint(0, 2, (BIG,), generator=g).to(dt)
    count = int((x != y).sum())
    want = np.float32(count) * (np.float32(1.0) / np.float32(BIG))
    return x, y, torch.tensor(want, dtype=FP32)


def emu_mse_fwd(x, y, defect=None):
    n, V = x.numel(), vec(x.dtype)
    grid = stream_grid(n, 8)
    threads = grid * KBLOCK
    nvec = n // V
    d = x.float() - y.float()
    trips = (nvec + threads - 1) // threads
    body = torch.zeros(trips * threads * V)
    body[: nvec * V] = d[: nvec * V]
    body = body.reshape(trips, threads, V)
    acc = torch.zeros(threads)
    for t in range(trips):
        for k in range(V):
            acc = fma32(body[t, :, k], body[t, :, k], acc)
    if defect != "skip_tail":
        tail = torch.zeros(threads)
        tail[: n - nvec * V] = d[nvec * V:]
        acc = fma32(tail, tail, acc)
    w = acc.reshape(grid, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):        # lane 0 of the shuffle tree
        w = w[..., :off] + w[..., off:2 * off]
    blocks = torch.zeros(grid)
    for i in range(4):
        blocks = blocks + w[:, i, 0]
    out = torch.zeros(())
    for b in range(grid):
        out = out + blocks[b]
    return out * float(np.float32(1.0) / np.float32(n))


@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_mse_fwd_emulation(dt):
    for n in flat_sizes(dt)[:-1]:
        x, y, ref, bound = mse_case(n, dt)
        r = worst(emu_mse_fwd(x, y), ref, bound)
        print(f"emu mse_fwd {dn(dt)} n={n}: {r:.3f}")
        assert r <= 1.0, (n, r)
        fb = BF.mse_loss(x, y)
        assert worst(fb, ref, bound) <= 1.0, n
    x, y, ref, bound = mse_case(vec(dt) + 1, dt)
    assert worst(emu_mse_fwd(x, y, "skip_tail"), ref, bound) >= 4.0
    x, y, want = mse_binary_case(dt)
    assert same_bits(emu_mse_fwd(x, y), want)
    assert not same_bits(emu_mse_fwd(x, y, "skip_tail"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=dn)
def test_mse_fwd_gpu(dt):
    top = 0.0
    for n in flat_sizes(dt):
        x, y, ref, bound = mse_case(n, dt)
        got = OPS.mse_fwd(x.to(DEV), y.to(DEV))
        assert got.dtype == FP32 and got.dim() == 0
        r = worst(got.cpu(), ref, bound)
        top = max(top, r)
        assert r <= 1.0, (dn(dt), n, r)
    print(f"gpu mse_fwd {dn(dt)}: {top:.3f}")
    x, y, want = mse_binary_case(dt)
    assert same_bits(OPS.mse_fwd(x.to(DEV), y.to(DEV)).cpu(), want)
    v = vec(dt)
    n = 4 * v - 1
    for p in (v + 1, n - 1):                # NaN locality: the loss is NaN
        x, y, _, _ = mse_case(n, dt)
        x = x.clone()
        x[p] = NAN
        assert bool(OPS.mse_fwd(x.to(DEV), y.to(DEV)).isnan())


# ---- host refusals ---------------------------------------------------------

def g(*shape, dt=FP32):
    return torch.ones(*shape, dtype=dt, device=DEV)


def refusals():
    """(call, message) pairs; nothing here may reach a kernel."""
    x = g(16)
    cpu = torch.ones(16)
    bf = g(16, dt=BF16)
    strided = g(32)[::2]
    short = g(15)
    out = []

    def second(op, call, name, first):
        for bad, why in ((cpu, f"on {first}'s device"), (bf, f"{first}'s dtype"),
                         (short, "elements"), (strided, "contiguous")):
            out.append((lambda bad=bad: call(bad), f"{op}: {name} must .*{why}"))

    second("relu_bwd", lambda t: OPS.relu_bwd(x, t), "y", "dy")
    second("gelu_bwd", lambda t: OPS.gelu_bwd(x, t), "x", "dy")
    second("add_relu_fwd", lambda t: OPS.add_relu_fwd(x, t), "b", "a")
    second("add_scaled_fwd", lambda t: OPS.add_scaled_fwd(x, t, 1.0), "b", "a")
    second("silu_mul_fwd", lambda t: OPS.silu_mul_fwd(x, t), "b", "a")
    second("silu_mul_bwd", lambda t: OPS.silu_mul_bwd(x, t, x), "a", "dy")
    second("silu_mul_bwd", lambda t: OPS.silu_mul_bwd(x, x, t), "b", "dy")
    second("mse_fwd", lambda t: OPS.mse_fwd(x, t), "y", "x")
    second("mse_bwd", lambda t: OPS.mse_bwd(x, t, g(1)), "y", "x")
    for op, call in (("relu_fwd", OPS.relu_fwd), ("gelu_fwd", OPS.gelu_fwd),
                     ("scale_fwd", lambda t: OPS.scale_fwd(t, 2.0))):
        out.append((lambda call=call: call(cpu), f"{op}: x must be on the GPU"))
        out.append((lambda call=call: call(strided), f"{op}: x must be contiguous"))
        out.append((lambda call=call: call(g(4).long()),
                    f"{op}: x must be fp32 or bf16"))

    def dout(op, call):
        for bad, why in ((torch.ones(1), "on"), (g(2), "1 elements"),
                         (g(1, dt=BF16), "fp32")):
            out.append((lambda bad=bad: call(bad), f"{op}: dout must .*{why}"))

    dout("mse_bwd", lambda d: OPS.mse_bwd(x, x, d))
    logits = g(4, 8)
    tgt = torch.zeros(4, dtype=torch.long, device=DEV)
    lse = g(4)
    dout("ce_bwd", lambda d: OPS.ce_bwd(logits, tgt, lse, d))
    for bad, why in ((tgt.cpu(), "on the logits' device"), (tgt.int(), "int64"),
                     (tgt[:3], "4 elements")):
        out.append((lambda bad=bad: OPS.ce_bwd(logits, bad, lse, g(1)),
                    f"ce_bwd: target must .*{why}"))
        out.append((lambda bad=bad: OPS.ce_fwd(logits, bad),
                    f"ce_fwd: target must .*{why}"))
    for bad, why in ((lse.cpu(), "on the logits' device"), (g(4, dt=BF16), "fp32"),
                     (g(5), "4 elements"), (g(8)[::2], "contiguous")):
        out.append((lambda bad=bad: OPS.ce_bwd(logits, tgt, bad, g(1)),
                    f"ce_bwd: lse must .*{why}"))
    out.append((lambda: OPS.ce_bwd(g(32), tgt, lse, g(1)),
                "ce_bwd: logits must be 2-D"))
    out.append((lambda: OPS.ce_fwd(g(32), tgt), "ce_fwd: logits must be 2-D"))

    for bad, why in ((cpu, "on {}'s device"), (bf, "fp32"), (short, "elements"),
                     (strided, "contiguous")):
        out.append((lambda bad=bad: OPS.scale_cast(bad, bf, 1.0),
                    "scale_cast: dst must .*" + why.format("src")))
        out.append((lambda bad=bad: OPS.cast_copy(bf, bad),
                    "cast_copy: src must .*" + why.format("dst")))
        out.append((lambda bad=bad: OPS.axpby(x, bad, 1.0, 1.0),
                    "axpby: x must .*" + why.format("y")))
    out.append((lambda: OPS.scale_cast(x, cpu, 1.0), "scale_cast: src must be on"))
    out.append((lambda: OPS.cast_copy(cpu, x), "cast_copy: dst must be on"))
    out.append((lambda: OPS.axpby(cpu, x, 1.0, 1.0), "axpby: y must be on"))
    out.append((lambda: OPS.axpby(bf, x, 1.0, 1.0), "axpby: y must be fp32"))
    out.append((lambda: OPS.axpby(strided, x, 1.0, 1.0),
                "axpby: y must be contiguous"))

    xr = g(2, 4, 3, 6)
    ct, st = g(4, 3), g(4, 3)
    out.append((lambda: OPS.rope(g(4, 3, 6), ct, st, False),
                "rope: x must be 4-D"))
    out.append((lambda: OPS.rope(g(2, 4, 3, 5), ct, st, False),
                "rope: x must have an even D"))
    out.append((lambda: OPS.rope(g(2, 4, 3, 0), ct, st, False),
                "rope: x must have an even D"))
    out.append((lambda: OPS.rope(xr.cpu(), ct, st, False),
                "rope: x must be on the GPU"))
    for name, call in (("cos_t", lambda t: OPS.rope(xr, t, st, False)),
                       ("sin_t", lambda t: OPS.rope(xr, ct, t, False))):
        for bad, why in ((ct.cpu(), "on x's device"), (g(4, 3, dt=BF16), "fp32"),
                         (g(12), "2-D"), (g(3, 3), "at least S = 4 rows"),
                         (g(4, 6), "exactly D / 2 = 3 columns"),
                         (g(4, 6)[:, ::2], "contiguous")):
            out.append((lambda bad=bad, call=call: call(bad),
                        f"rope: {name} must .*{why}"))
    out.append((lambda: OPS.rope(xr, g(5, 3), g(6, 3), False),
                "rope: sin_t must have cos_t's sizes"))

    out.append((lambda: OPS.colsum(g(())), "colsum: x must have at least one"))
    out.append((lambda: OPS.colsum(g(4, 0)), "colsum: x has C == 0"))
    out.append((lambda: OPS.colsum(g(0, 4)), "colsum: x has no rows"))
    out.append((lambda: OPS.colsum(cpu), "colsum: x must be on the GPU"))
    out.append((lambda: OPS.colsum(g(8, 8)[:, ::2]),
                "colsum: x must be contiguous"))
    out.append((lambda: OPS.transpose2d(x), "transpose2d: x must be 2-D"))
    out.append((lambda: OPS.transpose2d(g(8, 8).t()),
                "transpose2d: x must be contiguous"))
    out.append((lambda: OPS.transpose2d(torch.ones(4, 4)),
                "transpose2d: x must be on the GPU"))
    return out


@pytest.mark.gpu
def test_refusals_gpu():
    cases = refusals()
    assert len(cases) > 100
    for call, match in cases:
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()

"""LayerNorm, RMSNorm and BatchNorm (norm.hip) on every route, bf16 and
fp32, against float64 built from the stored inputs, with elementwise bounds
derived from the arithmetic (the form of tests/test_softmax_exact.py). The
route each case takes is asserted first: on the GPU what norm_route (the
csrc/norm_route.h the launchers execute) returns, against the tables below.

Notation: e = 2^-24 (one fp32 rounding), u = 2^-8 for a round-to-nearest bf16
store and 0 for fp32, n the number of summed terms (C for a LayerNorm /
RMSNorm row, M for a BatchNorm channel). A sum of n terms, in any order,
atomics included, errs by at most (n - 1) e sum|terms|; an fma chain by n e.
The plain count n is used, never the depth of today's reduction tree.
Second-order terms are covered by the +1 / +3 on n as long as n^2 e <= 1
(n <= 4096; the largest n here is 2056).

Statistics. All three families compute mean = sum/n and the variance in one
pass, var = sumsq/n - mean^2. With am = mean|x|, msq = mean(x^2):

    dmu  = (n + 1) e am                               sum, then one division
    dvar = (n + 3) e msq + 2 |mu| dmu + 2 e mu^2
           sumsq and its division: (n + 1) e msq; squaring the computed mean:
           2 |mu| dmu + dmu^2 + e mu^2; the subtraction: e var <= e msq
    t    = dvar / (var + eps)
    |rstd / ref - 1| <= drel = (1 - t)^-1/2 - 1 + 3 e
           the exact worst case of (var + eps - dvar)^-1/2, about t / 2, plus
           the add (e / 2), and v_rsq_f32's 1 ulp (2 e)

so the error of rstd grows with kappa = (msq + mu^2) / (var + eps): in the
kappa cases (mean of 8 sigma) |mu| dmu is about n e mu^2 and t about
1.5 n e kappa. RMSNorm has mu = dmu = 0 and var = msq: kappa is 1. mean and
rstd are fp32 outputs without a store term: |mean - ref| <= dmu and
|rstd - ref| <= ref drel are the sharp checks.

Forward. y = xhat w + b, xhat = (x - mu) rstd, pre = y before ReLU / store:

    |y - ref| <= u |ref| + (1 + u) A
    A = |w| (rstd (dmu + 2 e |mu|) + |xhat| (drel + 4 e)) + 2 e |b| [+ e |pre|]

rstd dmu and |xhat| drel propagate the statistics; 4 e |xhat w| covers the
subtraction, the two multiplies and the fma; the vectorized BatchNorm kernel
folds y = x K1 + K2, K1 = rstd gamma, K2 = beta - mean K1, which rounds
|mean K1| and |beta| once more each (2 e |mu|, 2 e |b|); the fused residual
add rounds pre once (e |pre|). ReLU is 1-Lipschitz, so the bound survives it,
and wherever pre < -A the output must be exactly 0. The store rounds the
computed value, not ref: hence (1 + u) A. running_mean / running_var are
checked against the float64 update rm0 + mom (mu - rm0) and
rv0 + mom (f var - rv0), f = M / (M - 1) (1 for M = 1):

    |rm - ref| <= mom dmu + e (|ref| + 2 mom |mu - rm0|)
    |rv - ref| <= mom (f dvar + 3 e (f var + |rv0|)) + e |ref|

Fused add (ln_add_fwd, rms_add_fwd). z must equal (x.float() + res.float())
.to(dtype) bit for bit; the reference is then taken from that z. The kernel
sums the unrounded fp32 z' and normalizes the rounded z, |z' - z| <= u' |z|
with u' = u / (1 - u). So the mean carries one extra u' am, and since
var(z') - var(z) = 2 cov(z, d) + var(d) with d = z' - z, Cauchy-Schwarz gives
the extra 2 u' sqrt(var msq) + u'^2 msq in dvar (the fp32 terms, now over z',
grow by (1 + u')^2). For fp32 u' = 0 and nothing changes.

Backward (LayerNorm / RMSNorm) takes the kernel's own mean / rstd as exact
inputs. g = dy w, m1 = mean(g) (0 for RMSNorm), m2 = mean(g xhat),
dx = rstd (g - m1 - xhat m2) [+ plus], G = |g| + |m1| + |xhat m2|:

    dm1 = (n + 1) e mean|g|,  dm2 = (n + 4) e mean|g xhat|   (xhat: 2 e, g: e)
    |dx - ref| <= u |ref| + (1 + u) (rstd (dm1 + |xhat| dm2 + 6 e G) [+ e |ref|])
    |dw - ref| <= (R + 3) e sum_r |dy xhat|,   |db - ref| <= R e sum_r |dy|

BatchNorm backward takes the kernel's own mean / rstd and stored y_post;
d = dy where y_post > 0 (all of dy without ReLU), s1 = sum d, s2 = sum d xhat,
g = rstd |gamma|, dx = rstd gamma (d - s1 / M - xhat s2 / M):

    |dbeta - ref| <= M e sum|d|,  |dgamma - ref| <= (M + 3) e sum|d xhat|
    |dx - ref| <= u |ref| + (1 + u) (g (ds1 / M + |xhat| ds2 / M)
                  + 8 e g (|d| + |s1 / M| + |xhat s2 / M|)
                  + 3 e g rstd |s2 / M| (|x| + |mean|))

the last term because the vectorized kernel expands (x - mean) K3 into
-x K3 + mean K3 and rounds each part. dres must equal the masked dy bit for
bit, and a channel that the ReLU masks entirely has s1 = s2 = 0, all bounds 0
and so dx, dgamma and dbeta exactly 0.

Inputs have unit variance, w / gamma = 1 + N(0, 1/4), b / beta = N(0, 1/4).
A count-based bound loosens with n, so |x| = |dy| = 16 is planted where an
indexing defect would lose data: the last column (last vector of the last
loop trip, last element of an odd tail, last channel of a partial chunk) of x
and dy for the row kernels, and the last row (of the last row block) of dy
for the column kernels and of x and dy for BatchNorm. Two cases carry no
outlier: (4, 768) has row means of 8 sigma (kappa = 65), and (6, 40) is scaled
by 2^-7 so that eps is a sixth of the variance and its placement matters.

The unmarked CPU test runs an fp32 emulation of each kernel family on the same
inputs: honest arithmetic must stay within 1.0 of every bound on every case,
each single-defect mutant must exceed 4x somewhere, and a truncating bf16
store (which can never reach 2) must exceed 1.5.

Worst observed error / bound over all cases and forms, on an MI355X and (in
parentheses) from the honest fp32 emulation on the CPU. Records, not
thresholds: the thresholds are 1.0 and the mutants' 4x. The bf16 y / dx
figures are the store term; the bf16 LayerNorm / RMSNorm mean and rstd
figures come from the fused-add forms (the u' terms), the plain forward stays
below 0.09 / 0.18.

    LayerNorm bf16   y 0.995 (0.995)  mean 0.680 (0.680)  rstd 0.731 (0.731)
                     dx 0.995 (0.995)  dw 0.399 (0.390)  db 0.157 (0.157)
    LayerNorm fp32   y 0.397 (0.397)  mean 0.062 (0.062)  rstd 0.095 (0.103)
                     dx 0.111 (0.151)  dw 0.394 (0.404)  db 0.460 (0.460)
    RMSNorm bf16     y 0.995 (0.995)  rstd 0.774 (0.774)
                     dx 0.996 (0.996)  dw 0.313 (0.289)
    RMSNorm fp32     y 0.159 (0.148)  rstd 0.163 (0.139)
                     dx 0.790 (0.795)  dw 0.315 (0.301)
    BatchNorm bf16   y 0.996 (0.996)  mean 0.068 (0.068)  rstd 0.223 (0.251)
                     running_mean 0.533 (0.568)  running_var 0.440 (0.413)
                     dx 0.995 (0.995)  dgamma 0.175 (0.128)  dbeta 0.016 (0.016)
    BatchNorm fp32   y 0.835 (0.843)  mean 0.173 (0.173)  rstd 0.195 (0.251)
                     running_mean 0.571 (0.571)  running_var 0.440 (0.413)
                     dx 0.254 (0.242)  dgamma 0.192 (0.126)  dbeta 0.173 (0.173)
    bn_fwd_eval      y 0.986 bf16, 0.638 fp32

In the kappa cases the one-pass variance sits far inside its bound (rstd at
0.001 of it for LayerNorm (4, 768), 0.009 for BatchNorm (256, 64)): the
bound counts n sequential roundings, the kernels sum in trees. z and dres
were bit-identical and every ReLU-masked output exactly 0 on every case."""

import functools

import pytest
import torch

if torch.cuda.is_available():
    from baton_amd.ops._ext import require_hip

    OPS = require_hip()
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
E = 2.0 ** -24
U = 2.0 ** -8
EPS = 1e-5
KMAXGRID = 2048
KBLOCK = 256
MOMENTUM = 0.3
INF = float("inf")


def dname(dt):
    return "bf16" if dt == BF16 else "fp32"


def vec_width(dt):
    return 8 if dt == BF16 else 4


# ---- routes: the CPU emulation's model of csrc/norm_route.h -------------------
# The GPU tests assert the tables below against norm_route itself;
# tests/test_norm_route.py holds these two functions equal to it.

def route_rows(R, C, dtype):
    """LayerNorm / RMSNorm. Row kernels: 16-byte vectors iff C % V == 0, 256
    threads stride the row, one block per row up to kMaxGrid blocks and
    grid-stride past it. Column kernels (dw / db): 64 channels x 4 row lanes
    per block, rows_per_block = max(128, ceil(R / (1024 / chunks))).
    Returns (vector, loop trips, grid capped, rows_per_block, grid.y)."""
    V = vec_width(dtype)
    vec = C % V == 0
    items = C // V if vec else C
    trips = -(-items // KBLOCK)
    chunks = (C + 63) // 64
    target = max(1, 1024 // chunks)
    rpb = max(128, -(-R // target))
    return (vec, trips, R > KMAXGRID, rpb, -(-R // rpb))


def route_bn(M, C, dtype):
    """BatchNorm. Stats kernels (forward and backward): vectorized iff
    C % 64 == 0, rows_per_block = max(64, ceil(M / (2048 / chunks))). The norm
    pass is vectorized iff C % V == 0 and C <= 6144, the dx pass iff C % V == 0
    and C <= 4096 (2 C and 3 C floats of LDS: 48 KiB at either limit); dres
    exists only on the vectorized dx pass. Both element loops run
    min(2048, ceil((M C / 4 + 1) / 256)) blocks of 256 threads over M C / V
    vectors (or M C elements) and grid-stride the rest.
    Returns (stats, rows_per_block, grid.y, norm, norm trips, dx, dx trips)."""
    V = vec_width(dtype)
    chunks = (C + 63) // 64
    target = max(1, 2048 // chunks)
    rpb = max(64, -(-M // target))
    gy = -(-M // rpb)
    threads = KBLOCK * max(1, min(KMAXGRID, -(-(M * C // 4 + 1) // KBLOCK)))
    norm_vec = C % V == 0 and C <= 6144
    dx_vec = C % V == 0 and C <= 4096
    nt = -(-(M * C // V if norm_vec else M * C) // threads)
    dt = -(-(M * C // V if dx_vec else M * C) // threads)
    return ("vec" if C % 64 == 0 else "scalar", rpb, gy,
            "vec" if norm_vec else "scalar", nt,
            "vec" if dx_vec else "scalar", dt)


# (R, C): {dtype: (vector, trips)}, grid capped, rows_per_block, grid.y.
# What each is for:
#   (5, 8)      one vector per row, 255 idle threads
#   (1, 768)    a single row
#   (3, 100)    vector for fp32, scalar for bf16; partial 64-channel chunk
#   (4, 1001)   scalar for both, several scalar trips
#   (3, 1028)   fp32: one vector into the second trip; bf16: scalar, 5 trips
#   (3, 2056)   bf16: one vector into the second trip; fp32: third trip
#   (130, 72)   column kernels with grid.y = 2, a last row block of 2 rows
#               (two idle row lanes), a partial channel chunk, atomics
#   (128, 64)   grid.y = 1: the direct-store branch
#   (2051, 64)  three rows past the 2048-block cap; grid.y = 17
#   (4, 768)    row means of 8 sigma: the one-pass variance at kappa = 65
#   (6, 40)     var = 6e-5: eps is a sixth of it
ROW_SHAPES = {
    (5, 8): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 1),
    (1, 768): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 1),
    (3, 100): ({BF16: (False, 1), FP32: (True, 1)}, False, 128, 1),
    (4, 1001): ({BF16: (False, 4), FP32: (False, 4)}, False, 128, 1),
    (3, 1028): ({BF16: (False, 5), FP32: (True, 2)}, False, 128, 1),
    (3, 2056): ({BF16: (True, 2), FP32: (True, 3)}, False, 128, 1),
    (130, 72): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 2),
    (128, 64): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 1),
    (2051, 64): ({BF16: (True, 1), FP32: (True, 1)}, True, 128, 17),
    (4, 768): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 1),  # kappa
    (6, 40): ({BF16: (True, 1), FP32: (True, 1)}, False, 128, 1),   # eps
}
KAPPA_ROWS = (4, 768)
EPS_ROWS = (6, 40)
ROW_CASES = [(R, C, dt) for (R, C) in ROW_SHAPES for dt in (BF16, FP32)]

# (M, C): {dtype: (norm, norm trips, dx, dx trips)}, stats, rows_per_block,
# grid.y, dtypes run. What each is for:
#   (1, 64)       M = 1: the guard on the unbiased variance
#   (37, 64)      vector stats, ragged 32-lane rows
#   (70, 72)      scalar stats with a partial chunk, two row blocks (the last
#                 of 6 rows: ragged 4-lane rows); vector norm / dx
#   (9, 12), (33, 100)   scalar stats; norm / dx vector for fp32, scalar
#                 (grid-strided) for bf16
#   (40, 4096)    vector norm and vector dx at the dx limit
#   (40, 4104)    vector norm, scalar dx
#   (40, 6144)    vector norm at its limit, scalar dx
#   (40, 6152)    scalar norm, scalar dx
#   (1032, 4096)  bf16 only: the vector element loops grid-stride once;
#                 grid.y = 17
#   (256, 64)     channel means of 8 sigma: kappa = 65; grid.y = 4
BN_SHAPES = {
    (1, 64): ({BF16: ("vec", 1, "vec", 1), FP32: ("vec", 1, "vec", 1)},
              "vec", 64, 1, (BF16, FP32)),
    (37, 64): ({BF16: ("vec", 1, "vec", 1), FP32: ("vec", 1, "vec", 1)},
               "vec", 64, 1, (BF16, FP32)),
    (70, 72): ({BF16: ("vec", 1, "vec", 1), FP32: ("vec", 1, "vec", 1)},
               "scalar", 64, 2, (BF16, FP32)),
    (9, 12): ({BF16: ("scalar", 1, "scalar", 1), FP32: ("vec", 1, "vec", 1)},
              "scalar", 64, 1, (BF16, FP32)),
    (33, 100): ({BF16: ("scalar", 4, "scalar", 4),
                 FP32: ("vec", 1, "vec", 1)}, "scalar", 64, 1, (BF16, FP32)),
    (40, 4096): ({BF16: ("vec", 1, "vec", 1), FP32: ("vec", 1, "vec", 1)},
                 "vec", 64, 1, (BF16, FP32)),
    (40, 4104): ({BF16: ("vec", 1, "scalar", 4),
                  FP32: ("vec", 1, "scalar", 4)}, "scalar", 64, 1,
                 (BF16, FP32)),
    (40, 6144): ({BF16: ("vec", 1, "scalar", 4),
                  FP32: ("vec", 1, "scalar", 4)}, "vec", 64, 1, (BF16, FP32)),
    (40, 6152): ({BF16: ("scalar", 4, "scalar", 4),
                  FP32: ("scalar", 4, "scalar", 4)}, "scalar", 64, 1,
                 (BF16, FP32)),
    (1032, 4096): ({BF16: ("vec", 2, "vec", 2)}, "vec", 64, 17, (BF16,)),
    (256, 64): ({BF16: ("vec", 1, "vec", 1), FP32: ("vec", 1, "vec", 1)},
                "vec", 64, 4, (BF16, FP32)),                       # kappa
}
KAPPA_BN = (256, 64)
BN_CASES = [(M, C, dt) for (M, C), v in BN_SHAPES.items() for dt in v[4]]


def case_id(c):
    return f"{c[0]}x{c[1]}_{dname(c[2])}"


ROW_KEYS = ("vec", "trips", "capped", "rows_per_block", "grid_y")
BN_KEYS = ("stats", "rows_per_block", "grid_y", "norm", "norm_trips", "dx",
           "dx_trips")


def launched_route(family, rows, C, dtype):
    """What the launchers execute, in the order of route_rows / route_bn."""
    d = OPS.norm_route(family, rows, C, dtype == BF16)
    return tuple(d[k] for k in (BN_KEYS if family == "bn" else ROW_KEYS))


def check_route_rows(R, C, dtype, family=None):
    """The table against the launchers' route (family given: GPU) or against
    the Python model."""
    per, capped, rpb, gy = ROW_SHAPES[(R, C)]
    want = per[dtype] + (capped, rpb, gy)
    got = launched_route(family, R, C, dtype) if family \
        else route_rows(R, C, dtype)
    assert got == want, (R, C, dname(dtype), got, want)


def check_route_bn(M, C, dtype, launched=False):
    per, stats, rpb, gy, _ = BN_SHAPES[(M, C)]
    n, nt, d, dt = per[dtype]
    want = (stats, rpb, gy, n, nt, d, dt)
    got = launched_route("bn", M, C, dtype) if launched \
        else route_bn(M, C, dtype)
    assert got == want, (M, C, dname(dtype), got, want)


# ---- inputs --------------------------------------------------------------------

def _pm16(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * 16.0


@functools.lru_cache(maxsize=2)
def row_inputs(R, C, dtype):
    """Stored x, res, dy, plus, w, b; never modified. z = x + res keeps the
    planted outlier of the last column (16 +- a few)."""
    g = torch.Generator().manual_seed(7919 * R + C)
    x = torch.randn(R, C, generator=g)
    res = torch.randn(R, C, generator=g)
    dy = torch.randn(R, C, generator=g)
    plus = torch.randn(R, C, generator=g)
    w = 1.0 + 0.5 * torch.randn(C, generator=g)
    b = 0.5 * torch.randn(C, generator=g)
    if (R, C) == KAPPA_ROWS:
        x += 8.0                      # row means of 8 sigma, no outliers
    elif (R, C) == EPS_ROWS:
        x *= 2.0 ** -7                # var = 6e-5: eps is a sixth of it
        res *= 2.0 ** -7
    else:
        x[:, -1] = _pm16((R,), g)
        dy[:, -1] = _pm16((R,), g)
        dy[-1, :] = _pm16((C,), g)
    return tuple(t.to(dtype) for t in (x, res, dy, plus, w, b))


@functools.lru_cache(maxsize=2)
def bn_inputs(M, C, dtype):
    """Stored x, res, dy (dtype) and fp32 gamma, beta, running_mean,
    running_var; never modified. Channel 3's beta is -100: with ReLU the whole
    channel is masked."""
    g = torch.Generator().manual_seed(104729 * M + C)
    x = torch.randn(M, C, generator=g)
    res = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    rm0 = torch.randn(C, generator=g)
    rv0 = 0.5 + torch.rand(C, generator=g)
    beta[3] = -100.0
    if (M, C) == KAPPA_BN:
        x += 8.0
    elif M > 1:
        x[-1, :] = _pm16((C,), g)
        dy[-1, :] = _pm16((C,), g)
    return (x.to(dtype), res.to(dtype), dy.to(dtype), gamma, beta, rm0, rv0)


# ---- float64 references and their bounds -----------------------------------------

def stats_bound(zd, dim, eps, center, u_add=0.0):
    """mu, var, rstd of zd over dim in float64 and dmu, dvar, drel (docstring).
    u_add: the statistics were summed over the unrounded z'."""
    n = zd.shape[dim]
    am = zd.abs().mean(dim, keepdim=True)
    msq = (zd * zd).mean(dim, keepdim=True)
    if center:
        mu = zd.mean(dim, keepdim=True)
        var = ((zd - mu) ** 2).mean(dim, keepdim=True)
        dmu = (n + 1) * E * am
    else:
        mu, var, dmu = torch.zeros_like(msq), msq, torch.zeros_like(msq)
    dvar = (n + 3) * E * msq + 2 * mu.abs() * dmu + 2 * E * mu * mu
    if u_add:
        up = u_add / (1 - u_add)
        dvar = (dvar * (1 + up) ** 2 + 2 * up * (var * msq).sqrt()
                + up * up * msq)
        if center:
            dmu = dmu * (1 + up) + up * am
    rstd = (var + eps) ** -0.5
    t = dvar / (var + eps)
    drel = torch.where(t < 1, (1 - t).clamp_min(1e-300) ** -0.5 - 1,
                       torch.full_like(t, INF)) + 3 * E
    return mu, var, rstd, dmu, dvar, drel


def fwd_refs(z, w, b, eps, dtype, dim, center, u_add=0.0, res=None,
             relu=False, given=None):
    """{'y', 'mean', 'rstd'}: (ref, bound), plus the statistics and
    (pre, A) for the exact-zero check. given = (mean, rstd): eval mode, the
    statistics are exact inputs."""
    u = U if dtype == BF16 else 0.0
    zd = z.double()
    if given is None:
        st = stats_bound(zd, dim, eps, center, u_add)
        mu, var, rstd, dmu, dvar, drel = st
    else:
        mu, rstd = (t.double().unsqueeze(dim) for t in given)
        dmu = drel = torch.zeros_like(mu)
        st = None
    wd = w.double()
    bd = torch.zeros_like(wd) if b is None else b.double()
    xhat = (zd - mu) * rstd
    pre = xhat * wd + bd
    A = (wd.abs() * (rstd * (dmu + 2 * E * mu.abs())
                     + xhat.abs() * (drel + 4 * E)) + 2 * E * bd.abs())
    if res is not None:
        pre = pre + res.double()
        A = A + E * pre.abs()
    ref = pre.clamp_min(0) if relu else pre
    out = {"y": (ref, u * ref.abs() + (1 + u) * A)}
    if given is None:
        out["rstd"] = (rstd.flatten(), (rstd * drel).flatten())
        if center:
            out["mean"] = (mu.flatten(), dmu.flatten())
    return out, st, (pre, A)


def running_refs(st, M, rm0, rv0, mom):
    mu, var, _, dmu, dvar, _ = (t.flatten() for t in st)
    f = M / (M - 1.0) if M > 1 else 1.0
    rm0, rv0 = rm0.double(), rv0.double()
    rm = rm0 + mom * (mu - rm0)
    rv = rv0 + mom * (f * var - rv0)
    return {
        "running_mean": (rm, mom * dmu + E * (rm.abs()
                                              + 2 * mom * (mu - rm0).abs())),
        "running_var": (rv, mom * (f * dvar + 3 * E * (f * var + rv0.abs()))
                        + E * rv.abs()),
    }


def rows_bwd_refs(x, dy, w, mean, rstd, plus, dtype, center):
    """LayerNorm / RMSNorm backward from the stored inputs and the given
    (the kernel's own) mean / rstd."""
    u = U if dtype == BF16 else 0.0
    R, C = x.shape
    rs = rstd.double()[:, None]
    mu = mean.double()[:, None] if center else 0.0
    xhat = (x.double() - mu) * rs
    dyd = dy.double()
    g = dyd * w.double()
    if center:
        m1 = g.mean(1, keepdim=True)
        dm1 = (C + 1) * E * g.abs().mean(1, keepdim=True)
    else:
        m1 = dm1 = torch.zeros(R, 1, dtype=torch.float64)
    m2 = (g * xhat).mean(1, keepdim=True)
    dm2 = (C + 4) * E * (g * xhat).abs().mean(1, keepdim=True)
    G = g.abs() + m1.abs() + (xhat * m2).abs()
    ref = rs * (g - m1 - xhat * m2)
    A = rs * (dm1 + xhat.abs() * dm2 + 6 * E * G)
    if plus is not None:
        ref = ref + plus.double()
        A = A + E * ref.abs()
    out = {"dx": (ref, u * ref.abs() + (1 + u) * A),
           "dw": ((dyd * xhat).sum(0), (R + 3) * E * (dyd * xhat).abs().sum(0))}
    if center:
        out["db"] = (dyd.sum(0), R * E * dyd.abs().sum(0))
    return out


def bn_bwd_refs(x, dy, y_post, mean, rstd, gamma, dtype, relu):
    u = U if dtype == BF16 else 0.0
    M, C = x.shape
    xd, mu, rs = x.double(), mean.double(), rstd.double()
    d = dy.double()
    if relu:
        d = torch.where(y_post.double() > 0, d, torch.zeros_like(d))
    xhat = (xd - mu) * rs
    s1, s2 = d.sum(0), (d * xhat).sum(0)
    ds1 = M * E * d.abs().sum(0)
    ds2 = (M + 3) * E * (d * xhat).abs().sum(0)
    m1, m2 = s1 / M, s2 / M
    g = rs * gamma.double().abs()
    ref = rs * gamma.double() * (d - m1 - xhat * m2)
    A = (g * (ds1 / M + xhat.abs() * ds2 / M)
         + 8 * E * g * (d.abs() + m1.abs() + (xhat * m2).abs())
         + 3 * E * g * rs * m2.abs() * (xd.abs() + mu.abs()))
    return {"dx": (ref, u * ref.abs() + (1 + u) * A),
            "dgamma": (s2, ds2), "dbeta": (s1, ds1)}, d


def worst(got, ref, lim):
    """max error / bound; anything non-finite, or any error where the bound
    is 0, counts as infinite."""
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs()
    r = torch.where(lim > 0, err / lim,
                    torch.where(err > 0, INF, 0.0).double())
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, INF))
    return r.max().item()


def ratios(prefix, outs, refs, into):
    for k, (ref, lim) in refs.items():
        key = prefix + k
        into[key] = max(into.get(key, 0.0), worst(outs[k], ref, lim))


def masked_exact(y, pre, A):
    """Where the reference is below zero by more than the error of pre, the
    ReLU output must be exactly 0; and it is never negative."""
    yd = y.double().reshape(pre.shape)
    return bool((yd[pre < -A] == 0).all() and (yd >= 0).all())


def report(tag, r):
    print(f"norm_exact {tag}: " + ", ".join(f"{k} {v:.4f}"
                                            for k, v in sorted(r.items())))


def assert_within(tag, r):
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: error / bound above 1: {bad}"


# ---- the cases, written once against an implementation ------------------------------
# impl is the GPU ops or the CPU emulation; both return CPU tensors in the
# bindings' order.

def run_rows(impl, family, R, C, dtype, mut=None, r=None):
    """Every form of one LayerNorm / RMSNorm case; returns {output: ratio}."""
    center = family == "ln"
    x, res, dy, plus, w, b = row_inputs(R, C, dtype)
    bb = b if center else None
    r = {} if r is None else r
    names = ("y", "mean", "rstd") if center else ("y", "rstd")

    out = impl.rows_fwd(family, x, None, w, bb, mut)
    refs, _, _ = fwd_refs(x, w, bb, EPS, dtype, 1, center)
    ratios("fwd.", dict(zip(names, out)), refs, r)
    mean, rstd = (out[1], out[2]) if center else (None, out[1])

    o2 = impl.rows_fwd(family, x, res, w, bb, mut)
    z = o2[1]
    z_want = (x.float() + res.float()).to(dtype)
    r["add.z_bits"] = 0.0 if torch.equal(z, z_want) else INF
    refs, _, _ = fwd_refs(z_want, w, bb, EPS, dtype, 1, center,
                          u_add=U if dtype == BF16 else 0.0)
    ratios("add.", dict(zip(names, (o2[0],) + tuple(o2[2:]))), refs, r)

    bnames = ("dx", "dw", "db") if center else ("dx", "dw")
    ob = impl.rows_bwd(family, x, dy, w, mean, rstd, None, mut)
    ratios("bwd.", dict(zip(bnames, ob)),
           rows_bwd_refs(x, dy, w, mean, rstd, None, dtype, center), r)
    ob = impl.rows_bwd(family, x, dy, w, mean, rstd, plus, mut)
    ratios("plus.", dict(zip(bnames, ob)),
           rows_bwd_refs(x, dy, w, mean, rstd, plus, dtype, center), r)
    return r


def dres_allowed(C, dtype):
    return C % vec_width(dtype) == 0 and C <= 4096


def run_bn(impl, M, C, dtype, mut=None, r=None, forms=("plain", "relu", "res")):
    """BatchNorm train forward (plain, fused ReLU, fused residual) with
    running statistics, and the backward of each from the implementation's own
    mean / rstd / y_post."""
    x, res, dy, gamma, beta, rm0, rv0 = bn_inputs(M, C, dtype)
    r = {} if r is None else r
    for form in forms:
        relu = form != "plain"
        rr = res if form == "res" else None
        y, mean, rstd, rm, rv = impl.bn_fwd(x, gamma, beta, rm0, rv0, MOMENTUM,
                                            relu, rr, mut)
        refs, st, (pre, A) = fwd_refs(x, gamma, beta, EPS, dtype, 0, True,
                                      res=rr, relu=relu)
        refs.update(running_refs(st, M, rm0, rv0, MOMENTUM))
        ratios(f"{form}.", {"y": y, "mean": mean, "rstd": rstd,
                            "running_mean": rm, "running_var": rv}, refs, r)
        if relu:
            r[f"{form}.masked_zero"] = 0.0 if masked_exact(y, pre, A) else INF
            assert (y[:, 3] == 0).all() or mut, "channel 3 is fully masked"
        want_dres = form == "res" and dres_allowed(C, dtype)
        if form == "res" and not want_dres:
            impl.bn_refuses_dres(x, dy, y, mean, rstd, gamma)
        ob = impl.bn_bwd(x, dy, y, mean, rstd, gamma, relu, want_dres, mut)
        brefs, d = bn_bwd_refs(x, dy, y, mean, rstd, gamma, dtype, relu)
        ratios(f"{form}.", dict(zip(("dx", "dgamma", "dbeta"), ob)), brefs, r)
        if want_dres:
            r["res.dres_bits"] = 0.0 if torch.equal(ob[3], d.to(dtype)) else INF
    return r


# ---- GPU ---------------------------------------------------------------------------

def _cpu(ts):
    return tuple(t.cpu() for t in ts)


class Gpu:
    @staticmethod
    def rows_fwd(family, x, res, w, b, mut=None):
        xd, wd = x.to(DEV), w.to(DEV)
        if family == "ln":
            if res is None:
                return _cpu(OPS.ln_fwd(xd, wd, b.to(DEV), EPS))
            return _cpu(OPS.ln_add_fwd(xd, res.to(DEV), wd, b.to(DEV), EPS))
        if res is None:
            return _cpu(OPS.rms_fwd(xd, wd, EPS))
        return _cpu(OPS.rms_add_fwd(xd, res.to(DEV), wd, EPS))

    @staticmethod
    def rows_bwd(family, x, dy, w, mean, rstd, plus, mut=None):
        a = [x.to(DEV), dy.to(DEV), w.to(DEV)]
        a += [mean.to(DEV), rstd.to(DEV)] if family == "ln" else [rstd.to(DEV)]
        if plus is not None:
            a.append(plus.to(DEV))
        name = ("ln" if family == "ln" else "rms") + \
            ("_bwd" if plus is None else "_bwd_plus")
        return _cpu(getattr(OPS, name)(*a))

    @staticmethod
    def bn_fwd(x, gamma, beta, rm0, rv0, mom, relu, res, mut=None):
        rm, rv = rm0.to(DEV), rv0.to(DEV)       # copies: updated in place
        y, mean, rstd = OPS.bn_fwd_train(
            x.to(DEV), gamma.to(DEV), beta.to(DEV), rm, rv, mom, EPS, relu,
            None if res is None else res.to(DEV))
        return _cpu((y, mean, rstd, rm, rv))

    @staticmethod
    def bn_bwd(x, dy, y_post, mean, rstd, gamma, relu, want_dres, mut=None):
        return _cpu(OPS.bn_bwd(x.to(DEV), dy.to(DEV), y_post.to(DEV),
                               mean.to(DEV), rstd.to(DEV), gamma.to(DEV), relu,
                               want_dres))

    @staticmethod
    def bn_refuses_dres(x, dy, y_post, mean, rstd, gamma):
        with pytest.raises(RuntimeError, match="dres"):
            OPS.bn_bwd(x.to(DEV), dy.to(DEV), y_post.to(DEV), mean.to(DEV),
                       rstd.to(DEV), gamma.to(DEV), True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROW_CASES, ids=case_id)
def test_layernorm(c):
    check_route_rows(*c, family="ln")
    r = run_rows(Gpu, "ln", *c)
    report("layernorm " + case_id(c), r)
    assert_within("layernorm " + case_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ROW_CASES, ids=case_id)
def test_rmsnorm(c):
    check_route_rows(*c, family="rms")
    r = run_rows(Gpu, "rms", *c)
    report("rmsnorm " + case_id(c), r)
    assert_within("rmsnorm " + case_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("c", BN_CASES, ids=case_id)
def test_batchnorm(c):
    check_route_bn(*c, launched=True)
    r = run_bn(Gpu, *c)
    report("batchnorm " + case_id(c), r)
    assert_within("batchnorm " + case_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=dname)
@pytest.mark.parametrize("shape", [(37, 64), (33, 100)], ids=str)
def test_batchnorm_eval(shape, dtype):
    """bn_fwd_eval normalizes with the given statistics: they are exact
    inputs, so only the rounding terms of the bound remain."""
    M, C = shape
    check_route_bn(M, C, dtype, launched=True)
    x, _, _, gamma, beta, rm0, rv0 = bn_inputs(M, C, dtype)
    rstd = (rv0 + EPS).rsqrt()
    r = {}
    for relu in (False, True):
        y = OPS.bn_fwd_eval(x.to(DEV), gamma.to(DEV), beta.to(DEV),
                            rm0.to(DEV), rstd.to(DEV), relu).cpu()
        refs, _, (pre, A) = fwd_refs(x, gamma, beta, EPS, dtype, 0, True,
                                     relu=relu, given=(rm0, rstd))
        ratios("relu." if relu else "plain.", {"y": y}, refs, r)
        if relu:
            r["relu.masked_zero"] = 0.0 if masked_exact(y, pre, A) else INF
    report(f"batchnorm_eval {M}x{C}_{dname(dtype)}", r)
    assert_within("batchnorm_eval", r)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=dname)
def test_batchnorm_without_running_stats(dtype):
    """Empty running-statistics tensors mean "absent": same y, mean and rstd,
    bit for bit, as with them."""
    M, C = 37, 64
    x, _, _, gamma, beta, rm0, rv0 = bn_inputs(M, C, dtype)
    a = (x.to(DEV), gamma.to(DEV), beta.to(DEV))
    none = OPS.bn_fwd_train(*a, torch.Tensor(), torch.Tensor(), MOMENTUM, EPS,
                            False, None)
    with_ = OPS.bn_fwd_train(*a, rm0.to(DEV), rv0.to(DEV), MOMENTUM, EPS,
                             False, None)
    for g, h in zip(none, with_):
        assert torch.equal(g, h)
    refs, _, _ = fwd_refs(x, gamma, beta, EPS, dtype, 0, True)
    r = {}
    ratios("", dict(zip(("y", "mean", "rstd"), _cpu(none))), refs, r)
    assert_within("batchnorm without running statistics", r)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=dname)
def test_batchnorm_fully_masked_channel(dtype):
    """beta[3] = -100 masks channel 3 entirely: sum_dy = sum_dyx = 0, and dx,
    dgamma, dbeta and dres of that channel are exactly 0."""
    M, C = 37, 64
    x, res, dy, gamma, beta, rm0, rv0 = bn_inputs(M, C, dtype)
    y, mean, rstd, _, _ = Gpu.bn_fwd(x, gamma, beta, rm0, rv0, MOMENTUM, True,
                                     res)
    assert (y[:, 3] == 0).all()
    dx, dgamma, dbeta, dres = Gpu.bn_bwd(x, dy, y, mean, rstd, gamma, True,
                                         True)
    assert (dx[:, 3] == 0).all() and (dres[:, 3] == 0).all()
    assert dgamma[3] == 0 and dbeta[3] == 0
    assert dgamma.abs().sum() > 0 and dx.float().abs().sum() > 0


# ---- GPU: host refusals ---------------------------------------------------------------

def _bad_variants(t, like_x):
    """(kind, tensor): wrong dtype, one row / element short, same sizes but
    not contiguous, on the CPU."""
    other = FP32 if t.dtype == BF16 else BF16
    if like_x:
        R, C = t.shape
        wide = torch.zeros(R, 2 * C, dtype=t.dtype, device=t.device)
        return [("dtype", t.to(other)), ("short", t[:-1].contiguous()
                                         if R > 1 else t[:, :-1].contiguous()),
                ("strided", wide[:, :C]), ("cpu", t.cpu())]
    n = t.numel()
    wide = torch.zeros(2 * n, dtype=t.dtype, device=t.device)
    return [("dtype", t.to(other)), ("short", t[:-1].contiguous()),
            ("long", torch.cat([t, t])), ("strided", wide[::2]),
            ("cpu", t.cpu())]


def _refusal_calls(dtype):
    """op -> (callable, ordered {arg name: tensor}, extra args, names of the
    x-like args, names checked)."""
    R, C = 6, 24
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)
    f32 = lambda *s: (0.5 + torch.rand(*s, generator=g)).to(DEV)
    x, res, dy, plus, yp = (mk(R, C) for _ in range(5))
    w, b = mk(C), mk(C)
    mean, rstd = f32(R), f32(R)
    gamma, beta, cm, cr, rm, rv = (f32(C) for _ in range(6))
    return {
        "ln_fwd": (dict(x=x, w=w, b=b), (EPS,), ()),
        "ln_add_fwd": (dict(x=x, res=res, w=w, b=b), (EPS,), ("res",)),
        "ln_bwd": (dict(x=x, dy=dy, w=w, mean=mean, rstd=rstd), (), ("dy",)),
        "ln_bwd_plus": (dict(x=x, dy=dy, w=w, mean=mean, rstd=rstd, plus=plus),
                        (), ("dy", "plus")),
        "rms_fwd": (dict(x=x, w=w), (EPS,), ()),
        "rms_add_fwd": (dict(x=x, res=res, w=w), (EPS,), ("res",)),
        "rms_bwd": (dict(x=x, dy=dy, w=w, rstd=rstd), (), ("dy",)),
        "rms_bwd_plus": (dict(x=x, dy=dy, w=w, rstd=rstd, plus=plus), (),
                         ("dy", "plus")),
        "bn_fwd_train": (dict(x=x, gamma=gamma, beta=beta, running_mean=rm,
                              running_var=rv, momentum=MOMENTUM, eps=EPS,
                              relu=True, res=res), (), ("res",)),
        "bn_fwd_eval": (dict(x=x, gamma=gamma, beta=beta, mean=cm, rstd=cr),
                        (False,), ()),
        "bn_bwd": (dict(x=x, dy=dy, y_post=yp, mean=cm, rstd=cr, gamma=gamma),
                   (True, False), ("dy", "y_post")),
    }


NORM_OPS = ("ln_fwd", "ln_add_fwd", "ln_bwd", "ln_bwd_plus", "rms_fwd",
            "rms_add_fwd", "rms_bwd", "rms_bwd_plus", "bn_fwd_train",
            "bn_fwd_eval", "bn_bwd")


def _call(op, args, extra):
    return getattr(OPS, op)(*args.values(), *extra)


def _unchanged(args, saved):
    return all(torch.equal(a, s) for a, s in zip(args.values(), saved)
               if isinstance(a, torch.Tensor))


def _saved(args):
    return [a.clone() if isinstance(a, torch.Tensor) else a
            for a in args.values()]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, FP32], ids=dname)
@pytest.mark.parametrize("op", NORM_OPS)
def test_norm_refuses_bad_arguments(op, dtype):
    """Every tensor argument but x, made wrong in one way at a time, is
    refused by name before anything is launched: the inputs are unchanged."""
    args, extra, like_x = _refusal_calls(dtype)[op]
    _call(op, dict(args), extra)                 # the good call is accepted
    torch.cuda.synchronize()
    saved = _saved(args)
    tried = 0
    for name, t in args.items():
        if name == "x" or not isinstance(t, torch.Tensor):
            continue
        for kind, bad in _bad_variants(t, name in like_x):
            a = dict(args)
            a[name] = bad
            with pytest.raises(RuntimeError, match=f"{op}: {name} "):
                _call(op, a, extra)
            tried += 1
    torch.cuda.synchronize()
    assert tried >= 5 and _unchanged(args, saved)

    # an x without rows or without channels
    for shape, what in (((0, 24), "no rows"), ((6, 0), "C == 0")):
        a = dict(args)
        a["x"] = torch.zeros(shape, dtype=dtype, device=DEV)
        with pytest.raises(RuntimeError, match=f"{op}: x has {what}"):
            _call(op, a, extra)
    assert _unchanged(args, saved)


@pytest.mark.gpu
def test_batchnorm_refuses_half_of_the_running_stats():
    args, extra, _ = _refusal_calls(BF16)["bn_fwd_train"]
    saved = _saved(args)
    for missing in ("running_mean", "running_var"):
        a = dict(args)
        a[missing] = torch.Tensor()
        with pytest.raises(RuntimeError,
                           match="running_mean and running_var must both"):
            _call("bn_fwd_train", a, extra)
    torch.cuda.synchronize()
    assert _unchanged(args, saved)


@pytest.mark.gpu
def test_batchnorm_y_post_is_only_read_with_relu():
    """Without ReLU y_post is not read, so it is not checked: callers pass an
    empty tensor."""
    args, _, _ = _refusal_calls(FP32)["bn_bwd"]
    a = dict(args)
    a["y_post"] = torch.Tensor()
    got = _call("bn_bwd", a, (False, False))
    want = _call("bn_bwd", args, (False, False))
    assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["ln_fwd", "ln_add_fwd", "ln_bwd",
                                "ln_bwd_plus"])
def test_layernorm_refuses_rows_past_int(op):
    """The LayerNorm kernels index rows with int: 2^31 rows are refused, not
    narrowed. (The check on x comes first, so the other arguments may be
    small.)"""
    x = torch.zeros(2 ** 31, 1, dtype=BF16, device=DEV)
    w = torch.ones(1, dtype=BF16, device=DEV)
    v = torch.ones(1, device=DEV)
    a = {"ln_fwd": (x, w, w, EPS), "ln_add_fwd": (x, x, w, w, EPS),
         "ln_bwd": (x, x, w, v, v), "ln_bwd_plus": (x, x, w, v, v, x)}[op]
    with pytest.raises(RuntimeError, match=f"{op}: x has 2147483648 rows"):
        getattr(OPS, op)(*a)
    torch.cuda.synchronize()
    assert not bool(x.any())


# ---- CPU: the bounds admit honest fp32 and reject single defects ------------------------

def _store(t, dtype, truncate=False):
    if dtype == FP32:
        return t
    if truncate:
        bits = t.contiguous().view(torch.int32) & -65536
        return bits.view(torch.float32).to(BF16)
    return t.to(BF16)


def _rows_kept(R, rpb, mut):
    if mut == "dropped_last_row":
        return R - 1
    if mut == "dropped_last_row_block":
        return (-(-R // rpb) - 1) * rpb
    return R


class Emu:
    """The kernels' arithmetic in fp32 on the CPU: one-pass variance, the
    same operation order, one store. mut names a single defect."""

    @staticmethod
    def rows_fwd(family, x, res, w, b, mut=None):
        center = family == "ln"
        dtype = x.dtype
        R, C = x.shape
        vec, _, capped, _, _ = route_rows(R, C, dtype)
        zf = x.float()
        z = None
        if res is not None:
            if mut != "res_not_added":
                zf = zf + res.float()
            z = zf.to(dtype)
        zr = zf if z is None else z.float()
        cols = C
        if mut == "dropped_last_vector" and vec:
            cols = C - vec_width(dtype)
        if mut == "dropped_tail_element" and not vec:
            cols = C - 1
        ss = (zf[:, :cols] * zf[:, :cols]).sum(1)
        if center:
            mu = zf[:, :cols].sum(1) / C
            var = ss / C - mu * mu
        else:
            mu = torch.zeros(R)
            var = ss / C
        var = var.clamp_min(0)
        rstd = 1.0 / (var.sqrt() + EPS) if mut == "eps_outside_sqrt" \
            else (var + EPS).rsqrt()
        y = (zr - mu[:, None]) * rstd[:, None] * w.float()
        if b is not None:
            y = y + b.float()
        y = _store(y, dtype, mut == "truncating_store")
        if mut == "no_grid_stride" and capped:
            y[KMAXGRID:] = float("nan")
        out = (y,) if z is None else (y, z)
        return out + ((mu, rstd) if center else (rstd,))

    @staticmethod
    def rows_bwd(family, x, dy, w, mean, rstd, plus, mut=None):
        center = family == "ln"
        dtype = x.dtype
        R, C = x.shape
        vec, _, _, rpb, _ = route_rows(R, C, dtype)
        rs = rstd[:, None]
        xhat = (x.float() - mean[:, None]) * rs if center else x.float() * rs
        dyf = dy.float()
        g = dyf * w.float()
        cols = C
        if mut == "dropped_last_vector" and vec:
            cols = C - vec_width(dtype)
        if mut == "dropped_tail_element" and not vec:
            cols = C - 1
        m1 = g[:, :cols].sum(1, keepdim=True) / C if center else 0.0
        m2 = (g * xhat)[:, :cols].sum(1, keepdim=True) / C
        if mut == "missing_m1":
            m1 = 0.0
        if mut == "missing_m2":
            m2 = 0.0
        dx = rs * (g - m1 - xhat * m2)
        if plus is not None and mut != "plus_not_added":
            dx = dx + plus.float()
        dx = _store(dx, dtype, mut == "truncating_store")
        rows = _rows_kept(R, rpb, mut)
        dw = (dyf * xhat)[:rows].sum(0)
        db = dyf[:rows].sum(0)
        if mut == "dropped_last_channel" and C % 64:
            dw[-1] = db[-1] = 0.0
        return (dx, dw, db) if center else (dx, dw)

    @staticmethod
    def bn_fwd(x, gamma, beta, rm0, rv0, mom, relu, res, mut=None):
        dtype = x.dtype
        M, C = x.shape
        _, rpb, _, _, _, _, _ = route_bn(M, C, dtype)
        xf = x.float()
        rows = _rows_kept(M, rpb, mut)
        s, ss = xf[:rows].sum(0), (xf[:rows] * xf[:rows]).sum(0)
        if mut == "dropped_last_channel" and C % 64:
            s[-1] = ss[-1] = 0.0
        mu = s / M
        var = (ss / M - mu * mu).clamp_min(0)
        rstd = 1.0 / (var.sqrt() + EPS) if mut == "eps_outside_sqrt" \
            else (var + EPS).rsqrt()
        unb = var * M / (M - 1) if M > 1 and mut != "biased_running_var" \
            else var
        rm = rm0 + mom * (mu - rm0)
        rv = rv0 + mom * (unb - rv0)
        gm = gamma.to(BF16).float() if mut == "bf16_gamma" else gamma
        k1 = rstd * gm
        k2 = beta - mu * k1
        y = xf * k1 + k2
        if res is not None and mut != "res_not_added":
            y = y + res.float()
        if relu:
            y = y.clamp_min(0)
        return (_store(y, dtype, mut == "truncating_store"), mu, rstd, rm, rv)

    @staticmethod
    def bn_bwd(x, dy, y_post, mean, rstd, gamma, relu, want_dres, mut=None):
        dtype = x.dtype
        M, C = x.shape
        _, rpb, _, _, _, _, _ = route_bn(M, C, dtype)
        xf, d = x.float(), dy.float()
        if relu:
            keep = (xf if mut == "relu_mask_from_x" else y_post.float()) > 0
            d = torch.where(keep, d, torch.zeros_like(d))
        xhat = (xf - mean) * rstd
        rows = _rows_kept(M, rpb, mut)
        s1, s2 = d[:rows].sum(0), (d * xhat)[:rows].sum(0)
        if mut == "dropped_last_channel" and C % 64:
            s1[-1] = s2[-1] = 0.0
        m1 = 0.0 if mut == "missing_m1" else s1 / M
        m2 = 0.0 if mut == "missing_m2" else s2 / M
        gm = gamma.to(BF16).float() if mut == "bf16_gamma" else gamma
        dx = rstd * gm * (d - m1 - xhat * m2)
        out = (_store(dx, dtype, mut == "truncating_store"), s2, s1)
        if want_dres:
            out += ((dy if mut == "dres_unmasked" else d.to(dtype)),)
        return out

    @staticmethod
    def bn_refuses_dres(*a):
        pass


ROW_MUTANTS = ("dropped_last_vector", "dropped_tail_element",
               "dropped_last_row", "dropped_last_row_block",
               "dropped_last_channel", "no_grid_stride", "missing_m1",
               "missing_m2", "plus_not_added", "res_not_added",
               "eps_outside_sqrt", "truncating_store")
BN_MUTANTS = ("dropped_last_row", "dropped_last_row_block",
              "dropped_last_channel", "biased_running_var", "missing_m1",
              "missing_m2", "relu_mask_from_x", "dres_unmasked",
              "res_not_added", "eps_outside_sqrt", "bf16_gamma",
              "truncating_store")


def _applies_rows(mut, family, R, C, dtype):
    vec, _, capped, rpb, gy = route_rows(R, C, dtype)
    return {"dropped_last_vector": vec, "dropped_tail_element": not vec,
            "dropped_last_row": True, "dropped_last_row_block": gy > 1,
            "dropped_last_channel": C % 64 != 0, "no_grid_stride": capped,
            "missing_m1": family == "ln",
            "truncating_store": dtype == BF16}.get(mut, True)


def _applies_bn(mut, M, C, dtype):
    gy = route_bn(M, C, dtype)[2]
    return {"dropped_last_row": M > 1, "dropped_last_row_block": gy > 1,
            "dropped_last_channel": C % 64 != 0,
            "biased_running_var": M > 1,
            "truncating_store": dtype == BF16}.get(mut, True)


def _top(r):
    return max(r.values())


@pytest.mark.parametrize("family", ["ln", "rms"])
def test_row_bounds_admit_fp32_and_reject_mutants(family):
    seen = {m: 0.0 for m in ROW_MUTANTS if family == "ln" or m != "missing_m1"}
    honest = {BF16: {}, FP32: {}}
    for c in ROW_CASES:
        R, C, dtype = c
        check_route_rows(R, C, dtype)
        r = run_rows(Emu, family, R, C, dtype)
        assert_within(f"honest {family} {case_id(c)}", r)
        for k, v in r.items():
            honest[dtype][k] = max(honest[dtype].get(k, 0.0), v)
        for m in seen:
            if _applies_rows(m, family, R, C, dtype):
                seen[m] = max(seen[m], _top(run_rows(Emu, family, R, C, dtype,
                                                     m)))
    for dt in (BF16, FP32):
        report(f"honest fp32 emulation {family} {dname(dt)}", honest[dt])
    print(f"norm_exact {family} mutants: {seen}")
    for m, v in seen.items():
        assert v > (1.5 if m == "truncating_store" else 4.0), (m, v)


def test_batchnorm_bounds_admit_fp32_and_reject_mutants():
    seen = {m: 0.0 for m in BN_MUTANTS}
    honest = {BF16: {}, FP32: {}}
    for c in BN_CASES:
        M, C, dtype = c
        check_route_bn(M, C, dtype)
        r = run_bn(Emu, M, C, dtype)
        assert_within(f"honest batchnorm {case_id(c)}", r)
        for k, v in r.items():
            honest[dtype][k] = max(honest[dtype].get(k, 0.0), v)
        if M * C > 300000:
            continue                 # the small shapes carry the mutants
        for m in seen:
            if _applies_bn(m, M, C, dtype):
                seen[m] = max(seen[m], _top(run_bn(Emu, M, C, dtype, m)))
    for dt in (BF16, FP32):
        report(f"honest fp32 emulation batchnorm {dname(dt)}", honest[dt])
    print(f"norm_exact batchnorm mutants: {seen}")
    for m, v in seen.items():
        assert v > (1.5 if m == "truncating_store" else 4.0), (m, v)

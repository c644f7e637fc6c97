"""Server optimizers over clipped client updates: FedAvgM, FedAdagrad,
FedAdam and FedYogi (Reddi et al., "Adaptive Federated Optimization").

Plain FedAvg moves parameters: ``theta = sum n_i theta_i / N``. Here the
federation moves bounded updates that a server-side step applies to an fp32
master copy ``x`` of the global model. Per round, with client i holding
``theta_i`` in its own dtype:

    w_i    = float32(n_i / N)
    d_i    = float(theta_i) - x
    norm_i = ||d_i|| over ALL averaged float tensors (parameters and float
             buffers), one norm per client
    f_i    = 1 if the sum of squares is finite, else 0
    c_i    = min(1, C / (norm_i + 1e-6))     (torch's clip_grad_norm_ rule;
             C = inf, "no clipping", gives exactly 1.0f)
    D      = sum_i (w_i c_i) d_i  over the clients with f_i = 1
    W      = sum_i w_i f_i,  inv_W = float32(1 / float64(W)),  Delta = D inv_W

A round with W not finite or not > 0 is skipped: x, m and v keep their bits,
``skipped_rounds`` goes up, and the clients are still handed x (a diverged
client is reset to the global model).

Server step on parameters, fp32, one rounding per operation, no bias
correction, m0 = 0, v0 = float32(tau * tau):

    fedavgm     m = fma(b1, m, Delta);                 x = fma(lr, m, x)
    adaptive    m = fma(b1, m, (1 - b1) Delta);        x = fma(lr, m / (sqrt(v) + tau), x)
      fedadagrad  v = fma(Delta, Delta, v)
      fedadam     v = fma(b2, v, (1 - b2) Delta Delta)
      fedyogi     d2 = Delta Delta;  v = v - (1 - b2) d2 sign(v - d2),  sign(0) = 0

Float buffers (BatchNorm statistics) take ``x = x + Delta`` with no momentum;
integer buffers are copied from the heaviest client, as in ``fedavg_``.

DP-FedAvg (McMahan et al., "Learning Differentially Private Recurrent
Language Models"), off unless ``dp_noise_multiplier`` z > 0; it needs a server
optimizer and a finite ``client_clip_norm`` C > 0. With w_i as above:

    sigma  = float32(z * C * max_i w_i)      (float64 on the host, rounded once)
    xi[e]  = fl(sigma * zeta[e])             zeta: the unit normal of element e
    Delta  = fl(D + xi)                      fixed denominator: NO multiply by inv_W

and Delta enters the unchanged step of each mode; float buffers are part of
the clipped norm, so they take the noise too. The denominator is the nominal
total weight 1 (DP-FedAvg's fixed-denominator estimator), so the number of
finite clients, which depends on the data, does not scale the released value.
A round with W not > 0 is still skipped and writes nothing. ``max_i w_i``
comes from the weights the host already holds.

Unit normals: Philox4x32-10 with the Random123 constants (multipliers
0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9, 0xBB67AE85). For flat
element index e within noise stream s, in round t:

    block j = e >> 2,  counter = (lo32(j), hi32(j), lo32(t), s),
    key = (lo32(seed), hi32(seed)),  output (r0, r1, r2, r3)
    u1 = ((r0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r1 >> 8) * 2^-24 in [0, 1)
    R = sqrtf(-2 logf(u1)),  zeta0 = R cospif(2 u2),  zeta1 = R sinpif(2 u2)
    zeta2, zeta3 likewise from (r2, r3); element e takes lane e & 3.

t counts every call of the round, skipped rounds included, so a (seed, t, s, e)
tuple is never reused. On the data plane s is the ordinal of the group in
``arena.all_groups`` and e the flat offset in the group; in ``ServerOptimizer``
s is the ordinal of the key among the float keys of ``global_sd`` and e the
offset in the tensor. The device evaluates the normals in fp32
(ops/csrc/fedopt.hip); the oracle here evaluates them in float64 from the same
integers (``unit_normals``) and rounds once to fp32.

Accounting: every registered client takes part in every round, so there is no
subsampling amplification. After T rounds, Renyi composition of the Gaussian
mechanism, min over alpha of alpha T / (2 z^2) + ln(1/delta) / (alpha - 1),
has the closed form ``privacy_spent``:

    eps(delta) = T / (2 z^2) + sqrt(2 T ln(1/delta)) / z

Limits of the guarantee, plainly: the client weights n_i are treated as
public. The skip of non-finite clients and of a whole round, and the integer
buffers copied from the heaviest client, are outside the guarantee. Philox is
not a cryptographic generator. The normal is a 24-bit discretisation truncated
at |zeta| <= sqrt(48 ln 2) ~ 5.77, and floating-point attacks on it are not
addressed. This is the level of the common DP training libraries in their
default mode, not a hardened one. The seed is never written to disk or to
metrics.

Robust aggregation (Yin et al., "Byzantine-Robust Distributed Learning";
FedMedian / FedTrimmedAvg), ``aggregator`` = "mean" (default: everything
above, untouched), "trimmed_mean" or "median"; ``trim_fraction`` beta in
[0, 0.5), default 0.1, is read only by "trimmed_mean". Per round:

    u_i   = fl(c_i * d_i)                       unweighted: n_i does not enter
    L     = { i : f_i = 1 },  k = |L|
    b(k)  = floor(float64(beta) * k)            trimmed_mean (float64 product, on the host)
          = (k - 1) // 2  (0 for k = 0)         median
    kept  = k - 2 b(k)                          (>= 1 whenever k >= 1)
    per element e: s_0 <= ... <= s_{k-1} = the sorted u_i[e], i in L
    S[e]  = fl(... fl(fl(s_b + s_{b+1}) + s_{b+2}) ... + s_{k-b-1})   ascending, one rounding per add
    Delta = fl(S * inv),  inv = float32(1 / float64(kept))

Delta enters the unchanged step of each mode; float buffers take
``x = x + Delta`` as above. A round with k = 0 is skipped exactly as a round
with W not > 0: nothing is written and ``skipped_rounds`` goes up. Live values
are finite by construction (a finite sum of squares implies finite elements),
so no NaN ordering is defined. Equal values, and -0.0 and +0.0, may leave the
sort in either order: results are defined by value, not by the sign bit of a
zero. With at most b(k) arbitrary finite rows among the k live ones, every
element of Delta lies within the range of the honest rows' values (up to the
rounding of the sum). What this does not cover: integer buffers still come
from the heaviest client, and n_i, which only that choice reads, is taken on
trust; a client that sends a non-finite update is dropped, which lowers k and
with it b(k). The rules are refused together with DP noise (their sensitivity
is not C max_i w_i, so the accounting above would be wrong) and with
``name == 'none'`` (``fedavgm`` with beta1 = 0 and lr = 1 is plain robust
FedAvg). ``trim_table`` builds b(0 .. K) once on the host; ``robust_delta`` is
the oracle of the device kernels (ops/csrc/fedrobust.hip).

This module is the CPU oracle of that definition (``ServerOptimizer.step_``,
what the HTTP manager runs) and holds the elementwise helpers the gloo branch
of the data plane shares; the HIP kernels (ops/csrc/fedopt.hip) run the same
operations in the same order on the device. An fma is formed here as the
float64 product and sum rounded to fp32: the product of two fp32 numbers is
exact in float64, so this differs from a true fma only by the double rounding
of the sum.
"""

from __future__ import annotations

import math
import secrets
from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

MODES = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")
ADAPTIVE = ("fedadagrad", "fedadam", "fedyogi")
# the step of a float buffer: x = x + Delta
MEAN = "mean"
# how the clients' updates become one Delta
AGGREGATORS = ("mean", "trimmed_mean", "median")


def f32(value: float) -> float:
    """``value`` rounded to fp32, as a Python float."""
    return torch.tensor(float(value), dtype=torch.float32).item()


def fma32(a, b, c: torch.Tensor) -> torch.Tensor:
    """fp32 fma(a, b, c) of fp32 operands (tensors or fp32-valued floats)."""
    a = a.double() if isinstance(a, torch.Tensor) else a
    b = b.double() if isinstance(b, torch.Tensor) else b
    return (a * b + c.double()).float()


def _t(value: float) -> torch.Tensor:
    return torch.tensor(value, dtype=torch.float32)


def clip_coef(sumsq: float, clip_norm: float):
    """(norm, coef, finite) from a client's sum of squares, in float64 with
    the coefficient rounded once to fp32: clip_finalize_kernel's rule."""
    finite = math.isfinite(sumsq)
    norm = math.sqrt(sumsq) if sumsq >= 0 else math.nan
    if not finite:
        return norm, 0.0, False
    return norm, f32(min(1.0, clip_norm / (norm + 1e-6))), True


def inv_weight(W: float):
    """(inv_W, applied) from the fp32 participation W."""
    applied = math.isfinite(W) and W > 0.0
    return (f32(1.0 / W) if applied else 0.0), applied


# ---- DP noise: Philox4x32-10, the unit normals and the accounting -------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 (Random123). ``counter`` is four and ``key`` two 32-bit
    words, each an int or an integer array (broadcast together); returns the
    four output words as uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & _MASK32 for w in key]
    if len(c) != 4 or len(k) != 2:
        raise ValueError("philox4x32 takes a 4-word counter and a 2-word key")
    m0, m1 = np.uint64(_PHILOX_M0), np.uint64(_PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]          # 32 x 32 -> 64 bits, exact
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _MASK32,
             (p0 >> s32) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & _MASK32,
             (k[1] + np.uint64(_PHILOX_W1)) & _MASK32]
    return tuple(w.astype(np.uint32) for w in c)


def _box_muller64(a: np.ndarray, b: np.ndarray):
    """The two normals of the words (a, b), in float64. cospi and sinpi are
    reduced by quadrant first, so their exact zeros are exact here too."""
    u1 = ((a >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    t = (b >> np.uint32(8)).astype(np.float64) * 2.0 ** -23     # 2 u2, exact
    with np.errstate(divide="ignore"):
        R = np.sqrt(-2.0 * np.log(u1))
    q = np.floor(2.0 * t)
    r = t - 0.5 * q                                              # [0, 1/2)
    c, s = np.cos(np.pi * r), np.sin(np.pi * r)
    cos = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    sin = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    return R * cos, R * sin


def unit_normals(seed: int, round: int, stream: int, offset: int,
                 n: int) -> np.ndarray:
    """zeta[offset .. offset + n) of stream ``stream`` in round ``round``:
    float64 from the integers the device uses (the module docstring)."""
    seed, round, stream, offset, n = (int(seed), int(round), int(stream),
                                      int(offset), int(n))
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    if round < 0 or not 0 <= stream < 2 ** 32 or offset < 0 or n < 0:
        raise ValueError("round, offset and n must be >= 0 and stream in "
                         "[0, 2^32)")
    if n == 0:
        return np.zeros(0, np.float64)
    j = np.arange(offset >> 2, ((offset + n - 1) >> 2) + 1, dtype=np.uint64)
    r = philox4x32((j & _MASK32, j >> np.uint64(32), round & 0xFFFFFFFF,
                    stream), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.stack(_box_muller64(r[0], r[1]) + _box_muller64(r[2], r[3]), axis=1)
    lo = offset & 3
    return np.ascontiguousarray(z.reshape(-1)[lo: lo + n])


def privacy_spent(rounds: int, noise_multiplier: float,
                  delta: float) -> float:
    """eps(delta) after ``rounds`` full-participation rounds with noise
    multiplier z: T / (2 z^2) + sqrt(2 T ln(1/delta)) / z, in float64."""
    T, z = float(rounds), float(noise_multiplier)
    if not 0.0 < delta < 1.0:
        raise ValueError(f"delta must be in (0, 1), got {delta}")
    if T < 0 or not z >= 0:
        raise ValueError("rounds and noise_multiplier must be >= 0")
    if T == 0:
        return 0.0
    if z == 0:
        return math.inf
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / delta)) / z


def dp_sigma(noise_multiplier: float, clip_norm: float,
             max_weight: float) -> float:
    """sigma = float32(z C max_i w_i), the product in float64."""
    return f32(float(noise_multiplier) * float(clip_norm) * float(max_weight))


def dp_xi(seed: int, round: int, stream: int, offset: int, n: int,
          sigma: float) -> torch.Tensor:
    """xi = fl(sigma * fl(zeta)) as an fp32 tensor of n elements."""
    zeta = torch.from_numpy(unit_normals(seed, round, stream, offset, n))
    return _t(sigma) * zeta.float()


# ---- robust aggregation: coordinate-wise median and trimmed mean ---------------


def trim_table(aggregator: str, beta: float, K: int) -> List[int]:
    """b(k) for k = 0 .. K: how many values are dropped at each end with k
    live clients (the module docstring). beta < 0.5 keeps 2 b(k) < k: the
    float64 product beta * k lies at least half a spacing below k / 2."""
    if aggregator not in AGGREGATORS or aggregator == "mean":
        raise ValueError(
            f"trim_table: aggregator must be trimmed_mean or median, got "
            f"{aggregator!r}")
    K = int(K)
    if K < 0:
        raise ValueError(f"trim_table: K must be >= 0, got {K}")
    if aggregator == "median":
        return [0 if k == 0 else (k - 1) // 2 for k in range(K + 1)]
    beta = float(beta)
    if not 0.0 <= beta < 0.5:
        raise ValueError(
            f"server_opt.trim_fraction must be in [0, 0.5), got {beta}")
    return [int(math.floor(beta * k)) for k in range(K + 1)]


def robust_counts(flags, table: Sequence[int]):
    """(k, b, kept, inv, applied) from the clients' flags and ``trim_table``'s
    table: robust_finalize_kernel's rule."""
    flags = [bool(f) for f in flags]
    if len(table) != len(flags) + 1:
        raise ValueError(
            f"the trim table must have {len(flags) + 1} entries, got "
            f"{len(table)}")
    k = sum(flags)
    applied = k > 0
    b = int(table[k]) if applied else 0
    b = min(max(b, 0), (k - 1) // 2 if applied else 0)
    kept = k - 2 * b
    return k, b, kept, (f32(1.0 / kept) if applied else 0.0), applied


def robust_sum(U: torch.Tensor, flags, table: Sequence[int]) -> torch.Tensor:
    """S: per element the ascending sequential fp32 sum of the sorted live
    rows of ``U`` ([K, n] fp32) from rank b to rank k - b - 1. Dead rows are
    never read. Zeros with k = 0."""
    if U.dim() != 2 or U.dtype != torch.float32:
        raise ValueError("robust_sum: U must be a 2-D fp32 tensor")
    if U.shape[0] != len(flags):
        raise ValueError("robust_sum: one flag per row of U")
    k, b, kept, _, applied = robust_counts(flags, table)
    S = torch.zeros(U.shape[1], dtype=torch.float32)
    if not applied:
        return S
    live = [i for i, f in enumerate(flags) if bool(f)]
    s = torch.sort(U.detach().to("cpu")[live], dim=0).values
    S.copy_(s[b])
    for j in range(b + 1, k - b):
        S = S + s[j]                 # fp32, one rounding per add
    return S


def robust_delta(U: torch.Tensor, flags,
                 table: Sequence[int]) -> Optional[torch.Tensor]:
    """Delta = fl(S * inv) of the live rows of ``U``, or None for a round
    without a live row (k = 0: the round is skipped)."""
    _, _, _, inv, applied = robust_counts(flags, table)
    if not applied:
        return None
    return robust_sum(U, flags, table) * _t(inv)


def server_update_(mode: str, D: torch.Tensor, inv_w: float, x: torch.Tensor,
                   m: Optional[torch.Tensor], v: Optional[torch.Tensor],
                   lr: float, b1: float, b2: float, tau: float) -> None:
    """One applied server step on fp32 tensors, in place; lr, b1, b2, tau are
    fp32-valued. The order of operations is server_step_kernel's."""
    server_apply_(mode, D * _t(inv_w), x, m, v, lr, b1, b2, tau)


def server_apply_(mode: str, delta: torch.Tensor, x: torch.Tensor,
                  m: Optional[torch.Tensor], v: Optional[torch.Tensor],
                  lr: float, b1: float, b2: float, tau: float) -> None:
    """The step of ``server_update_`` from Delta itself (fl(D inv_W), or
    fl(D + xi) with DP noise)."""
    if mode == MEAN:
        x.add_(delta)
        return
    if mode == "fedavgm":
        m.copy_(fma32(b1, m, delta))
        x.copy_(fma32(lr, m, x))
        return
    m.copy_(fma32(b1, m, _t(f32(1.0 - b1)) * delta))
    omb2 = _t(f32(1.0 - b2))
    if mode == "fedadagrad":
        v.copy_(fma32(delta, delta, v))
    elif mode == "fedadam":
        v.copy_(fma32(b2, v, omb2 * delta * delta))
    elif mode == "fedyogi":
        d2 = delta * delta
        v.copy_(v - omb2 * d2 * torch.sign(v - d2))
    else:
        raise ValueError(f"unknown server optimizer {mode!r}")
    x.copy_(fma32(lr, m / (torch.sqrt(v) + _t(tau)), x))


def validate(name: str, lr: float, beta1: float, beta2: float, tau: float,
             client_clip_norm: float, dp_noise_multiplier: float = 0.0,
             dp_seed: Optional[int] = None, dp_delta: float = 1e-5,
             aggregator: str = "mean", trim_fraction: float = 0.1) -> None:
    if name != "none" and name not in MODES:
        raise ValueError(
            f"unknown server optimizer {name!r} (none, {', '.join(MODES)})")
    if aggregator not in AGGREGATORS:
        raise ValueError(
            f"unknown server_opt.aggregator {aggregator!r} "
            f"({', '.join(AGGREGATORS)})")
    if not 0.0 <= trim_fraction < 0.5:
        raise ValueError(
            f"server_opt.trim_fraction must be in [0, 0.5), got "
            f"{trim_fraction}")
    if aggregator != "mean":
        if name == "none":
            raise ValueError(
                f"server_opt.aggregator {aggregator!r} needs a server "
                "optimizer (name is 'none'): fedavgm with beta1 = 0 and "
                "lr = 1 is plain robust FedAvg")
        if dp_noise_multiplier != 0:
            raise ValueError(
                f"server_opt.aggregator {aggregator!r} cannot be combined "
                "with dp_noise_multiplier > 0: the sensitivity of a robust "
                "rule is not C max_i w_i, so the privacy accounting would be "
                "wrong")
    if not lr > 0:
        raise ValueError(f"server_opt.lr must be > 0, got {lr}")
    for label, b in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"server_opt.{label} must be in [0, 1), got {b}")
    if not tau > 0 and (name in ADAPTIVE or tau != tau):
        raise ValueError(f"server_opt.tau must be > 0, got {tau}")
    if not client_clip_norm >= 0:
        raise ValueError(
            f"server_opt.client_clip_norm must be >= 0 (0 = off), got "
            f"{client_clip_norm}")
    z = dp_noise_multiplier
    if z == 0:
        return
    if not (z > 0 and math.isfinite(z)):
        raise ValueError(
            f"server_opt.dp_noise_multiplier must be finite and >= 0, got {z}")
    if name == "none":
        raise ValueError(
            "server_opt.dp_noise_multiplier > 0 needs a server optimizer "
            "(name is 'none')")
    if not (client_clip_norm > 0 and math.isfinite(client_clip_norm)):
        raise ValueError(
            "server_opt.dp_noise_multiplier > 0 needs a finite "
            f"client_clip_norm > 0, got {client_clip_norm}")
    if not 0.0 < dp_delta < 1.0:
        raise ValueError(
            f"server_opt.dp_delta must be in (0, 1), got {dp_delta}")
    if dp_seed is not None and not (
            isinstance(dp_seed, int) and 0 <= dp_seed < 2 ** 64):
        raise ValueError(
            f"server_opt.dp_seed must be an integer in [0, 2^64), got "
            f"{dp_seed}")


def resolve_seed(dp_seed: Optional[int]) -> int:
    """``dp_seed``, or a fresh 64-bit seed from ``secrets`` for None."""
    return secrets.randbits(64) if dp_seed is None else int(dp_seed)


class ServerOptimizer:
    """The server step on CPU state dicts, with its own fp32 master copy of
    every float tensor. ``client_clip_norm`` 0 (or inf) means no clipping.
    ``noise_multiplier`` > 0 turns DP-FedAvg on (the module docstring):
    ``seed`` None draws a fresh one, ``dp_rounds`` counts the calls of
    ``step_`` made with it, skipped rounds included. ``aggregator``
    "trimmed_mean" (with ``trim_fraction``) or "median" combines the clients
    coordinate-wise instead; ``last_live`` and ``last_trimmed`` are then the
    last round's k and b(k)."""

    def __init__(self, name: str = "fedavgm", lr: float = 1.0,
                 beta1: float = 0.9, beta2: float = 0.99, tau: float = 1e-3,
                 client_clip_norm: float = 0.0, noise_multiplier: float = 0.0,
                 seed: Optional[int] = None, delta: float = 1e-5,
                 aggregator: str = "mean", trim_fraction: float = 0.1):
        validate(name, lr, beta1, beta2, tau, client_clip_norm,
                 noise_multiplier, seed, delta, aggregator, trim_fraction)
        # "mean", or a robust rule (the module docstring): then the last
        # round's live clients k and trim b(k) are last_live, last_trimmed
        self.aggregator = aggregator
        self.trim_fraction = float(trim_fraction)
        self.last_live = 0
        self.last_trimmed = 0
        self.noise_multiplier = float(noise_multiplier)
        self.delta = float(delta)
        self.seed = resolve_seed(seed) if self.noise_multiplier > 0 else None
        self.dp_rounds = 0
        self.last_sigma = 0.0
        if name == "none":
            raise ValueError("'none' is plain FedAvg: there is no optimizer")
        self.name = name
        self.lr, self.beta1, self.beta2, self.tau = (
            f32(lr), f32(beta1), f32(beta2), f32(tau))
        self.client_clip_norm = (
            float(client_clip_norm) if client_clip_norm > 0 else math.inf)
        self.x: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self.m: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self.v: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self.skipped_rounds = 0
        # the last round's per-client figures and participation
        self.norm: List[float] = []
        self.coef: List[float] = []
        self.finite: List[bool] = []
        self.last_W = 0.0
        self.applied = True
        # the last round's reduced update per key and 1 / W (0 when skipped)
        self.last_D: Dict[str, torch.Tensor] = {}
        self.last_inv_W = 0.0

    @classmethod
    def from_config(cls, cfg) -> Optional["ServerOptimizer"]:
        """A ServerOptConfig -> optimizer, or None for ``name == 'none'``."""
        if cfg is None or cfg.name == "none":
            return None
        return cls(cfg.name, cfg.lr, cfg.beta1, cfg.beta2, cfg.tau,
                   cfg.client_clip_norm, cfg.dp_noise_multiplier, cfg.dp_seed,
                   cfg.dp_delta, getattr(cfg, "aggregator", "mean"),
                   getattr(cfg, "trim_fraction", 0.1))

    @property
    def epsilon(self) -> float:
        """eps(delta) spent so far; 0.0 with DP off."""
        if self.noise_multiplier <= 0:
            return 0.0
        return privacy_spent(self.dp_rounds, self.noise_multiplier, self.delta)

    # -- state -----------------------------------------------------------------

    def _ensure_state(self, global_sd, param_names: Iterable[str]) -> None:
        params = set(param_names)
        for k, t in global_sd.items():
            if not t.is_floating_point() or k in self.x:
                continue
            self.x[k] = t.detach().to("cpu", torch.float32).clone()
            if k in params:
                self.m[k] = torch.zeros_like(self.x[k])
                if self.name in ADAPTIVE:
                    self.v[k] = torch.full_like(
                        self.x[k], f32(self.tau * self.tau))

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Flat tensors: ``x.<key>``, ``m.<key>``, ``v.<key>`` and the
        0-dim int64 ``skipped_rounds``; with DP noise on, the 0-dim int64
        ``dp_rounds`` as well (never the seed)."""
        out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        out["skipped_rounds"] = torch.tensor(self.skipped_rounds,
                                             dtype=torch.int64)
        if self.noise_multiplier > 0:
            out["dp_rounds"] = torch.tensor(self.dp_rounds, dtype=torch.int64)
        for prefix, d in (("x", self.x), ("m", self.m), ("v", self.v)):
            for k, t in d.items():
                out[f"{prefix}.{k}"] = t.clone()
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        x, m, v = OrderedDict(), OrderedDict(), OrderedDict()
        dest = {"x": x, "m": m, "v": v}
        skipped = 0
        dp_rounds = 0
        for k, t in sd.items():
            if k == "skipped_rounds":
                skipped = int(t.item())
                continue
            if k == "dp_rounds":
                dp_rounds = int(t.item())
                continue
            prefix, _, key = k.partition(".")
            if prefix not in dest or not key:
                raise KeyError(f"unexpected server optimizer state key {k!r}")
            if t.dtype != torch.float32:
                raise ValueError(f"server optimizer state {k!r} must be fp32")
            dest[prefix][key] = t.detach().to("cpu").clone()
        self.x, self.m, self.v = x, m, v
        self.skipped_rounds = skipped
        self.dp_rounds = dp_rounds

    # -- the round ---------------------------------------------------------------

    def step_(
        self,
        global_sd: "OrderedDict[str, torch.Tensor]",
        client_sds: Sequence["OrderedDict[str, torch.Tensor]"],
        weights: Sequence[float],
        param_names: Iterable[str],
    ) -> "OrderedDict[str, torch.Tensor]":
        """One federated round into ``global_sd``, in place. ``weights`` are
        the clients' n_samples; ``param_names`` the keys that take the
        optimizer step (every other float key is a buffer)."""
        if len(client_sds) == 0:
            raise ValueError("step_ needs at least one client state_dict")
        if len(client_sds) != len(weights):
            raise ValueError("client_sds and weights length mismatch")
        total = float(sum(weights))
        if total <= 0:
            raise ValueError("total weight must be positive")
        params = set(param_names)
        self._ensure_state(global_sd, params)
        fkeys = [k for k, t in global_sd.items() if t.is_floating_point()]
        for sd in client_sds:
            for k in global_sd:
                if k not in sd:
                    raise KeyError(f"client state_dict missing key {k!r}")

        if self.aggregator != "mean":
            self._robust_round(client_sds, fkeys, params)
            return self._install(global_sd, client_sds, weights)

        noisy = self.noise_multiplier > 0
        if noisy:
            t = self.dp_rounds
            self.dp_rounds += 1          # every call, skipped rounds included
            self.last_sigma = dp_sigma(
                self.noise_multiplier, self.client_clip_norm,
                max(f32(float(n_i) / total) for n_i in weights))
        self.norm, self.coef, self.finite = [], [], []
        D = {k: torch.zeros_like(self.x[k]) for k in fkeys}
        W = _t(0.0)
        for sd, n_i in zip(client_sds, weights):
            w_i = f32(float(n_i) / total)
            deltas = {
                k: sd[k].detach().to("cpu", torch.float32) - self.x[k]
                for k in fkeys
            }
            sumsq = sum(float(d.double().pow(2).sum()) for d in deltas.values())
            norm, coef, finite = clip_coef(sumsq, self.client_clip_norm)
            self.norm.append(norm)
            self.coef.append(coef)
            self.finite.append(finite)
            if not finite:
                continue           # contributes +0.0 and weight 0
            s = _t(w_i) * _t(coef)
            for k in fkeys:
                D[k] += s * deltas[k]
            W = W + _t(w_i)
        self.last_W = W.item()
        inv_w, self.applied = inv_weight(self.last_W)
        self.last_D, self.last_inv_W = D, inv_w
        if self.applied:
            for s, k in enumerate(fkeys):
                mode = self.name if k in params else MEAN
                if noisy:
                    xi = dp_xi(self.seed, t, s, 0, D[k].numel(),
                               self.last_sigma).reshape(D[k].shape)
                    delta = D[k] + xi
                else:
                    delta = D[k] * _t(inv_w)
                server_apply_(mode, delta, self.x[k], self.m.get(k),
                              self.v.get(k), self.lr, self.beta1, self.beta2,
                              self.tau)
        else:
            self.skipped_rounds += 1
        return self._install(global_sd, client_sds, weights)

    def _robust_round(self, client_sds, fkeys: List[str], params) -> None:
        """The round of a robust aggregator on x, m, v: the clients' clipped,
        unweighted updates u_i = c_i d_i, per key the kept sum over the
        sorted live clients, Delta = S / kept into the unchanged step."""
        self.norm, self.coef, self.finite = [], [], []
        rows: Dict[str, List[torch.Tensor]] = {k: [] for k in fkeys}
        for sd in client_sds:
            deltas = {
                k: sd[k].detach().to("cpu", torch.float32) - self.x[k]
                for k in fkeys
            }
            sumsq = sum(float(d.double().pow(2).sum()) for d in deltas.values())
            norm, coef, finite = clip_coef(sumsq, self.client_clip_norm)
            self.norm.append(norm)
            self.coef.append(coef)
            self.finite.append(finite)
            for k in fkeys:
                # a dead client's row is never read: zeros stand in for it
                rows[k].append((_t(coef) * deltas[k]).reshape(-1) if finite
                               else torch.zeros(deltas[k].numel()))
        table = trim_table(self.aggregator, self.trim_fraction,
                           len(client_sds))
        k_live, b, kept, inv, self.applied = robust_counts(self.finite, table)
        self.last_live, self.last_trimmed = k_live, b
        self.last_W, self.last_inv_W = float(kept), inv
        self.last_D = {}
        if not self.applied:
            self.skipped_rounds += 1
            return
        for k in fkeys:
            S = robust_sum(torch.stack(rows[k]), self.finite, table)
            self.last_D[k] = S.reshape(self.x[k].shape)
            mode = self.name if k in params else MEAN
            server_apply_(mode, self.last_D[k] * _t(inv), self.x[k],
                          self.m.get(k), self.v.get(k), self.lr, self.beta1,
                          self.beta2, self.tau)

    def _install(self, global_sd, client_sds, weights):
        """x into ``global_sd`` in its dtypes; integer buffers from the
        heaviest client."""
        heaviest = max(range(len(weights)), key=lambda i: weights[i])
        for k, gt in global_sd.items():
            if gt.is_floating_point():
                gt.detach().copy_(self.x[k].to(gt.dtype))
            else:
                gt.detach().copy_(client_sds[heaviest][k].to(device=gt.device))
        return global_sd

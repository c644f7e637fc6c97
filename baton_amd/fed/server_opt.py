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
from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Sequence

import torch

MODES = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")
ADAPTIVE = ("fedadagrad", "fedadam", "fedyogi")
# the step of a float buffer: x = x + Delta
MEAN = "mean"


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


def server_update_(mode: str, D: torch.Tensor, inv_w: float, x: torch.Tensor,
                   m: Optional[torch.Tensor], v: Optional[torch.Tensor],
                   lr: float, b1: float, b2: float, tau: float) -> None:
    """One applied server step on fp32 tensors, in place; lr, b1, b2, tau are
    fp32-valued. The order of operations is server_step_kernel's."""
    delta = D * _t(inv_w)
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
             client_clip_norm: float) -> None:
    if name != "none" and name not in MODES:
        raise ValueError(
            f"unknown server optimizer {name!r} (none, {', '.join(MODES)})")
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


class ServerOptimizer:
    """The server step on CPU state dicts, with its own fp32 master copy of
    every float tensor. ``client_clip_norm`` 0 (or inf) means no clipping."""

    def __init__(self, name: str = "fedavgm", lr: float = 1.0,
                 beta1: float = 0.9, beta2: float = 0.99, tau: float = 1e-3,
                 client_clip_norm: float = 0.0):
        validate(name, lr, beta1, beta2, tau, client_clip_norm)
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
                   cfg.client_clip_norm)

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
        0-dim int64 ``skipped_rounds``."""
        out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        out["skipped_rounds"] = torch.tensor(self.skipped_rounds,
                                             dtype=torch.int64)
        for prefix, d in (("x", self.x), ("m", self.m), ("v", self.v)):
            for k, t in d.items():
                out[f"{prefix}.{k}"] = t.clone()
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        x, m, v = OrderedDict(), OrderedDict(), OrderedDict()
        dest = {"x": x, "m": m, "v": v}
        skipped = 0
        for k, t in sd.items():
            if k == "skipped_rounds":
                skipped = int(t.item())
                continue
            prefix, _, key = k.partition(".")
            if prefix not in dest or not key:
                raise KeyError(f"unexpected server optimizer state key {k!r}")
            if t.dtype != torch.float32:
                raise ValueError(f"server optimizer state {k!r} must be fp32")
            dest[prefix][key] = t.detach().to("cpu").clone()
        self.x, self.m, self.v = x, m, v
        self.skipped_rounds = skipped

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
            for k in fkeys:
                mode = self.name if k in params else MEAN
                server_update_(mode, D[k], inv_w, self.x[k], self.m.get(k),
                               self.v.get(k), self.lr, self.beta1, self.beta2,
                               self.tau)
        else:
            self.skipped_rounds += 1

        heaviest = max(range(len(weights)), key=lambda i: weights[i])
        for k, gt in global_sd.items():
            if gt.is_floating_point():
                gt.detach().copy_(self.x[k].to(gt.dtype))
            else:
                gt.detach().copy_(client_sds[heaviest][k].to(device=gt.device))
        return global_sd

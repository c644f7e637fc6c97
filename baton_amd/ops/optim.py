"""Fused optimizers.

The reference's optimizer is stock ``torch.optim.SGD`` driven per-batch
(/root/reference/demo.py:34,47). Here the step is a hand-written gfx950 HIP
kernel (csrc/optim.hip): one launch per contiguous buffer, fp32 math, with
momentum / weight-decay / Adam variants — and when the model's parameters
live in a FlatParamArena (runtime/arena.py) the whole step is ONE kernel
over one flat buffer, sized for HBM3E streaming (vectorized float4 access).

CPU fallback uses torch._foreach so the control-plane tests run GPU-free;
on a GPU box the HIP kernel is mandatory (ops/_ext.require_hip).
"""

from __future__ import annotations

import math
from typing import Iterable, List, Optional

import torch

from baton_amd.ops._ext import require_hip
from baton_amd.utils.config import TrainConfig


def _collect(params: Iterable[torch.nn.Parameter]) -> List[torch.nn.Parameter]:
    out = [p for p in params if p.requires_grad]
    if not out:
        raise ValueError("optimizer got an empty parameter list")
    return out


class _FusedOptimizerBase:
    """Steps either a list of nn.Parameters (one kernel per tensor) or a
    FlatParamArena (ONE kernel per dtype group — the production path)."""

    def __init__(self, params=None, arena=None, max_grad_norm=None,
                 decoupled_weight_decay=False):
        self.arena = arena
        if arena is not None:
            # (flat_params, flat_grads) per dtype group
            self.params = [g.flat for g in arena.groups]
            self._arena_grads = [g.grad for g in arena.groups]
            self.device = self.params[0].device
        else:
            self.params = _collect(params)
            self._arena_grads = None
            self.device = self.params[0].device
        self._use_hip = self.device.type == "cuda"
        # Arena + HIP: the step kernel writes zeros back to the flat grad
        # after consuming it (zero_grad fused), so zero_grad() is a no-op
        # (arena grads start zeroed; backward accumulates into them).
        self._fused_zero = self._use_hip and arena is not None
        if self._use_hip:
            require_hip()  # fail loudly up front, not at step N
        self._init_clip(max_grad_norm, decoupled_weight_decay)

    # -- global-norm clipping, non-finite skip, decoupled decay --------------

    def _init_clip(self, max_grad_norm, decoupled_weight_decay) -> None:
        """``max_grad_norm`` (None = off, ``float('inf')`` = measure and skip
        non-finite steps without clipping) clips the GLOBAL gradient norm —
        one norm over all dtype groups of an arena, or over all tensors of a
        parameter list — by torch's ``clip_grad_norm_`` rule
        ``coef = min(1, max_norm / (norm + 1e-6))``. A step whose squared norm
        is not finite (an inf or NaN anywhere in the gradients) is skipped:
        parameters and moments keep their bits, ``skipped_steps()`` goes up.

        Norm, coef and the skip decision live in ``clip_state`` on the device
        ([norm, coef, finite, skipped]); ``step()`` never reads them on the
        host, and everything it needs is allocated here, so a captured graph
        carries the whole sequence."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(
                    f"max_grad_norm must be > 0 (or None), got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        # the dense ops run unless one of the two is asked for
        self._ext = max_grad_norm is not None or self.decoupled_weight_decay
        self.clip_state = None
        self._partials = None
        self._partial_offsets: List[int] = []
        self._partial_counts: List[int] = []
        if max_grad_norm is None:
            return
        self.clip_state = torch.zeros(4, dtype=torch.float32, device=self.device)
        if self._use_hip:
            ops = require_hip()
            # one slot per block of each buffer's grad_sumsq grid
            total = 0
            for p in self.params:
                self._partial_offsets.append(total)
                self._partial_counts.append(int(ops.optim_grid(p.numel())))
                total += self._partial_counts[-1]
            self._partials = torch.zeros(
                total, dtype=torch.float32, device=self.device)

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """The last step's global gradient norm before clipping: a device
        scalar (a view of ``clip_state[0]``), None without ``max_grad_norm``."""
        return None if self.clip_state is None else self.clip_state[0]

    def skipped_steps(self) -> int:
        """Steps skipped so far for a non-finite gradient (a host read)."""
        return 0 if self.clip_state is None else int(self.clip_state[3].item())

    def _measure_hip(self, ops, grads) -> None:
        """One grad_sumsq per buffer, one clip_finalize; no host read. Every
        buffer owns fixed slots of the partials; one without a gradient has
        its slots zeroed so that it adds nothing."""
        count = 0
        for g, off, n in zip(grads, self._partial_offsets, self._partial_counts):
            if g is None:
                self._partials[off:off + n].zero_()
            else:
                ops.grad_sumsq(g, self._partials, off)
            count = off + n
        ops.clip_finalize(self._partials, count, self.max_grad_norm,
                          self.clip_state)

    def _measure_cpu(self, grads) -> Optional[torch.Tensor]:
        """The fallback's clip_state; returns coef (a 0-dim fp32 tensor), or
        None when the step must be skipped."""
        sumsq = torch.zeros((), dtype=torch.float32)
        for g in grads:
            if g is not None:
                sumsq = sumsq + g.float().pow(2).sum()
        norm = sumsq.sqrt()
        finite = bool(torch.isfinite(sumsq))
        coef = torch.clamp(self.max_grad_norm / (norm.double() + 1e-6),
                           max=1.0).float() if finite else torch.zeros(())
        self.clip_state[0] = norm
        self.clip_state[1] = coef
        self.clip_state[2] = 1.0 if finite else 0.0
        if not finite:
            self.clip_state[3] += 1.0
        return coef if finite else None

    def zero_grad(self, set_to_none: bool = True) -> None:
        if self.arena is not None:
            if not self._fused_zero:
                self.arena.zero_grads()
            return
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    def _grads(self) -> List[Optional[torch.Tensor]]:
        if self._arena_grads is not None:
            return self._arena_grads
        return [p.grad for p in self.params]


class FusedSGD(_FusedOptimizerBase):
    """SGD with optional momentum + weight decay, one HIP kernel per buffer.

    Semantics match torch.optim.SGD (and therefore the reference demo):
        g = grad + wd * p
        m = mu * m + g          (momentum buffer, if mu > 0)
        p = p - lr * (m if mu>0 else g)

    ``max_grad_norm`` clips the global norm and skips non-finite steps (see
    ``_FusedOptimizerBase._init_clip``); g above is then coef * grad.
    ``decoupled_weight_decay`` replaces the L2 term by p *= 1 - lr * wd in
    front of the update. With neither, ``step()`` calls ``sgd_step`` as ever.
    """

    def __init__(
        self,
        params: Optional[Iterable[torch.nn.Parameter]] = None,
        lr: float = 1e-3,
        momentum: float = 0.0,
        weight_decay: float = 0.0,
        arena=None,
        max_grad_norm: Optional[float] = None,
        decoupled_weight_decay: bool = False,
    ):
        super().__init__(params, arena, max_grad_norm, decoupled_weight_decay)
        self.lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        self.momentum_bufs: List[Optional[torch.Tensor]] = [
            torch.zeros_like(p, dtype=torch.float32) if momentum > 0 else None
            for p in self.params
        ]

    @classmethod
    def from_arena(cls, arena, **kw):
        return cls(arena=arena, **kw)

    @torch.no_grad()
    def step(self) -> None:
        grads = self._grads()
        if self._use_hip and self._ext:
            ops = require_hip()
            if self.clip_state is not None:
                self._measure_hip(ops, grads)
            for p, g, m in zip(self.params, grads, self.momentum_bufs):
                if g is None:
                    continue
                ops.sgd_step_ext(
                    p.data if isinstance(p, torch.nn.Parameter) else p,
                    g,
                    m if m is not None else torch.empty(0, device=self.device),
                    self.lr,
                    self.momentum,
                    self.weight_decay,
                    self._fused_zero,
                    self.clip_state,
                    self.decoupled_weight_decay,
                )
            return
        if self._use_hip:
            ops = require_hip()
            for p, g, m in zip(self.params, grads, self.momentum_bufs):
                if g is None:
                    continue
                ops.sgd_step(
                    p.data if isinstance(p, torch.nn.Parameter) else p,
                    g,
                    m if m is not None else torch.empty(0, device=self.device),
                    self.lr,
                    self.momentum,
                    self.weight_decay,
                    self._fused_zero,
                )
            return
        # CPU fallback (same math)
        coef = None
        if self.clip_state is not None:
            coef = self._measure_cpu(grads)
            if coef is None:
                return  # non-finite gradients: the step is skipped
        for p, g, m in zip(self.params, grads, self.momentum_bufs):
            if g is None:
                continue
            gf = g.float()
            if coef is not None:
                gf = gf * coef
            if self.weight_decay and self.decoupled_weight_decay:
                p.data.add_(p.data, alpha=-self.lr * self.weight_decay)
            elif self.weight_decay:
                gf = gf.add(p.data.float(), alpha=self.weight_decay)
            if self.momentum > 0:
                m.mul_(self.momentum).add_(gf)
                gf = m
            p.data.add_(gf.to(p.dtype), alpha=-self.lr)


class FusedAdam(_FusedOptimizerBase):
    """Adam (bias-corrected), one HIP kernel per buffer; fp32 moments.

    Semantics match torch.optim.Adam:
        m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
        p -= lr * (m / (1-b1^t)) / (sqrt(v / (1-b2^t)) + eps)
    with decoupled-free weight decay (L2: g += wd * p), like torch's Adam.

    ``decoupled_weight_decay=True`` is torch.optim.AdamW: p *= 1 - lr * wd in
    front of the update and no L2 term. ``max_grad_norm`` clips the global
    norm and skips non-finite steps (``_FusedOptimizerBase._init_clip``); g
    above is then coef * grad. With neither, ``step()`` calls ``adam_step`` as
    ever.

    ``step_count`` is a host counter and the skip is decided on the device, so
    it advances on a skipped step too: after a skip the bias correction runs
    one step ahead of the moments (1 - b^t taken at t + 1), an error that
    fades like b^t.
    """

    def __init__(
        self,
        params: Optional[Iterable[torch.nn.Parameter]] = None,
        lr: float = 1e-3,
        betas=(0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 0.0,
        arena=None,
        max_grad_norm: Optional[float] = None,
        decoupled_weight_decay: bool = False,
    ):
        super().__init__(params, arena, max_grad_norm, decoupled_weight_decay)
        self.lr = lr
        self.beta1, self.beta2 = betas
        self.eps = eps
        self.weight_decay = weight_decay
        self.step_count = 0
        self.exp_avg = [torch.zeros_like(p, dtype=torch.float32) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, dtype=torch.float32) for p in self.params]

    @classmethod
    def from_arena(cls, arena, **kw):
        return cls(arena=arena, **kw)

    @torch.no_grad()
    def step(self) -> None:
        self.step_count += 1
        bc1 = 1.0 - self.beta1**self.step_count
        bc2 = 1.0 - self.beta2**self.step_count
        grads = self._grads()
        if self._use_hip and self._ext:
            ops = require_hip()
            if self.clip_state is not None:
                self._measure_hip(ops, grads)
            for p, g, m, v in zip(self.params, grads, self.exp_avg, self.exp_avg_sq):
                if g is None:
                    continue
                ops.adam_step_ext(
                    p.data if isinstance(p, torch.nn.Parameter) else p,
                    g, m, v,
                    self.lr, self.beta1, self.beta2, self.eps,
                    self.weight_decay, bc1, bc2, self._fused_zero,
                    self.clip_state, self.decoupled_weight_decay,
                )
            return
        if self._use_hip:
            ops = require_hip()
            for p, g, m, v in zip(self.params, grads, self.exp_avg, self.exp_avg_sq):
                if g is None:
                    continue
                ops.adam_step(
                    p.data if isinstance(p, torch.nn.Parameter) else p,
                    g, m, v,
                    self.lr, self.beta1, self.beta2, self.eps,
                    self.weight_decay, bc1, bc2, self._fused_zero,
                )
            return
        coef = None
        if self.clip_state is not None:
            coef = self._measure_cpu(grads)
            if coef is None:
                return  # non-finite gradients: the step is skipped
        for p, g, m, v in zip(self.params, grads, self.exp_avg, self.exp_avg_sq):
            if g is None:
                continue
            gf = g.float()
            if coef is not None:
                gf = gf * coef
            if self.weight_decay and self.decoupled_weight_decay:
                p.data.add_(p.data, alpha=-self.lr * self.weight_decay)
            elif self.weight_decay:
                gf = gf.add(p.data.float(), alpha=self.weight_decay)
            m.mul_(self.beta1).add_(gf, alpha=1 - self.beta1)
            v.mul_(self.beta2).addcmul_(gf, gf, value=1 - self.beta2)
            denom = (v / bc2).sqrt_().add_(self.eps)
            p.data.add_((m / bc1 / denom).to(p.dtype), alpha=-self.lr)


def make_optimizer(params: Iterable[torch.nn.Parameter], cfg: TrainConfig):
    # TrainConfig.max_grad_norm: 0 means off
    max_grad_norm = cfg.max_grad_norm if cfg.max_grad_norm else None
    if cfg.optimizer == "sgd":
        return FusedSGD(
            params, lr=cfg.lr, momentum=cfg.momentum,
            weight_decay=cfg.weight_decay, max_grad_norm=max_grad_norm,
        )
    if cfg.optimizer in ("adam", "adamw"):
        return FusedAdam(
            params,
            lr=cfg.lr,
            betas=tuple(cfg.adam_betas),
            eps=cfg.adam_eps,
            weight_decay=cfg.weight_decay,
            max_grad_norm=max_grad_norm,
            decoupled_weight_decay=cfg.optimizer == "adamw",
        )
    raise ValueError(f"unknown optimizer {cfg.optimizer!r}")

"""RCCL-over-xGMI data plane: the FedAvg theta-traffic fast path.

The reference moves every round's parameters twice through the manager's
single TCP socket as pickled CPU tensors (SURVEY.md §2.3/§5 — fine for
Linear(10,1), catastrophic for ResNet/BERT). Here the 8 GPUs of one MI355X
node are 8 federated clients, one process per GPU (`torch.distributed`,
backend "nccl" = RCCL on ROCm), and the theta traffic is:

    pre-scaled REDUCE to the root GPU  +  BROADCAST of the new global model

which matches the FedAvg semantics exactly (Sum n_i * theta_i on root, scale
by 1/N — reference manager.py:119-126) and suits the xGMI topology: links
are point-to-point (7 x ~153 GB/s per GPU), so the naturally-rooted
reduce/broadcast pair is used instead of translating an all-reduce pattern
designed for switched fabrics.

Overlap (overlap_stream=True, GPU+nccl only): the whole aggregation runs on
a side HIP stream, bucketed. Each bucket's pre-scale (HIP scale_cast) and
cast-back (cast_copy) execute on the side stream while the RCCL reduce /
broadcast of the *previous* bucket is still in flight on the communicator's
own stream (async_op collectives; xGMI link time hides under the fused
casts, and vice versa). The compute stream is fenced with HIP events: it
waits for aggregation-complete only at `PendingAggregation.wait()` — or at
the end of `fedavg_arena` when called synchronously — so the next round's
parameter-independent work (grad zero-fill, input staging, host-side
bookkeeping) proceeds while theta traffic is still on the wire.

Numerics: the reduce runs in fp32 regardless of model dtype (config
reduce_dtype), so the result is comparable against the CPU/HTTP FedAvg
oracle; tests assert near-bit-exact agreement in fp32.

Server optimizer (`enable_server_opt` + `fedopt_arena`, off by default): the
ranks send clipped updates w_i c_i (theta_i - x) against an fp32 master x
where FedAvg sends parameters, rank 0 applies FedAvgM / FedAdagrad / FedAdam /
FedYogi to x between the reduce and the broadcast (ops/csrc/fedopt.hip), and
every rank installs x. Same streams, buckets and fence; the definition and
the CPU oracle are in fed/server_opt.py. With `dp_noise_multiplier` > 0 rank
0's step adds DP-FedAvg noise in the same pass (`server_step_noise` with
rank 0's seed, the round index, the group ordinal as stream and the bucket's
start as element offset); `dp_rounds` counts every round, skipped ones
included, and `dp_epsilon` reports the privacy spent. With `aggregator`
'trimmed_mean' or 'median' the ranks send unweighted clipped updates, rank 0
gathers them bucket by bucket into staging rows and `robust_select`
(ops/csrc/fedrobust.hip) writes their coordinate-wise kept sum where the
reduce would have left D; the step, the broadcast and the cast are the same.

CPU testing: the same class runs on gloo with world_size>1 (reduce/broadcast
are identical calls), which is how tests/test_data_plane.py exercises the
distributed path without a GPU.
"""

from __future__ import annotations

import logging
import os
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from baton_amd.runtime.arena import FlatParamArena
from baton_amd.utils.config import DataPlaneConfig
from baton_amd.utils.tracing import trace_scope

log = logging.getLogger("baton.dataplane")

# Bucket size for the overlapped aggregation pipeline (elements of fp32).
# 16 MiB buckets: large enough that each RCCL call is bandwidth-bound on a
# single xGMI link (~153 GB/s per direction), small enough that the fused
# scale/cast of bucket i+1 has real link time to hide under.
_BUCKET_ELEMS = 4 * 1024 * 1024


class PendingAggregation:
    """Handle for an in-flight (side-stream) federated aggregation.

    `wait()` fences the CALLER's current stream against aggregation
    completion (no host sync). Anything enqueued on the compute stream
    before `wait()` overlaps the collectives; the first op that reads the
    averaged parameters must come after it."""

    def __init__(self, weights: torch.Tensor, done_event=None):
        self.weights = weights
        self._done = done_event
        self._waited = done_event is None

    def wait(self) -> torch.Tensor:
        if not self._waited:
            torch.cuda.current_stream().wait_event(self._done)
            self._waited = True
        return self.weights


class FederatedDataPlane:
    """One instance per rank (= per GPU-client). Rank 0 is the aggregation
    root — the "manager GPU"."""

    def __init__(
        self,
        config: Optional[DataPlaneConfig] = None,
        device: Optional[torch.device] = None,
    ):
        self.config = config or DataPlaneConfig()
        if not dist.is_initialized():
            self._init_from_env()
        self.rank = dist.get_rank()
        self.world_size = dist.get_world_size()
        if device is not None:
            self.device = device
        elif torch.cuda.is_available():
            self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", self.rank % max(torch.cuda.device_count(), 1))))
        else:
            self.device = torch.device("cpu")
        self._side_stream: Optional[torch.cuda.Stream] = None
        if self.device.type == "cuda" and self.config.overlap_stream:
            self._side_stream = torch.cuda.Stream(device=self.device)
        self._reduce_bufs: dict = {}
        # handle for the most recent aggregation (set by fedavg_arena)
        self.pending: Optional[PendingAggregation] = None
        # (graph, captured weights, captured n_samples) from capture_aggregation
        self._agg_graph = None
        # state of fedopt_arena (enable_server_opt); None = plain FedAvg
        self._fedopt: Optional[dict] = None

    def _init_from_env(self) -> None:
        backend = self.config.backend
        if backend == "nccl" and not torch.cuda.is_available():
            backend = "gloo"
        os.environ.setdefault("MASTER_ADDR", self.config.master_addr)
        os.environ.setdefault("MASTER_PORT", str(self.config.master_port))
        dist.init_process_group(backend=backend)
        log.info(
            "data plane up: backend=%s rank=%d/%d",
            backend,
            dist.get_rank(),
            dist.get_world_size(),
        )

    # -- collectives -----------------------------------------------------------

    def gather_weights(self, n_samples: int) -> torch.Tensor:
        """All-gather every client's sample count -> fp64 [world] tensor
        (tiny; the FedAvg weights)."""
        t = torch.tensor([float(n_samples)], dtype=torch.float64, device=self._coll_device())
        out = [torch.zeros_like(t) for _ in range(self.world_size)]
        dist.all_gather(out, t)
        return torch.cat(out).cpu()

    def _coll_device(self) -> torch.device:
        # gloo wants CPU tensors; nccl/RCCL wants device tensors
        if dist.get_backend() == "gloo":
            return torch.device("cpu")
        return self.device

    def fedavg_flat(
        self, flat: torch.Tensor, n_samples: int, weights: Optional[torch.Tensor] = None
    ) -> torch.Tensor:
        """In-place federated average of a flat tensor across all ranks.

        Every rank ends up with the new global value (reduce to root 0 in
        fp32, scale by 1/N on root, broadcast). Returns the gathered weight
        vector for reuse (loss-history weighting, heaviest-rank policy).
        """
        if weights is None:
            weights = self.gather_weights(n_samples)
        total = float(weights.sum().item())
        if total <= 0:
            raise ValueError("total sample weight must be positive")
        scale = float(n_samples) / total

        src = flat.reshape(-1)
        assert src.is_contiguous(), "fedavg_flat needs a contiguous flat tensor"
        buf = self._reduce_buf(src.numel())
        if buf.device.type == "cuda" and src.device == buf.device:
            if self._side_stream is not None:
                # overlapped path: pipeline on the side stream, fence here
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
                with torch.cuda.stream(self._side_stream):
                    self._side_stream.wait_event(ev)
                    self._fedavg_gpu_pipelined(src, buf, scale)
                    done = torch.cuda.Event()
                    done.record(self._side_stream)
                torch.cuda.current_stream().wait_event(done)
            else:
                self._fedavg_gpu_pipelined(src, buf, scale)
        else:
            buf.copy_(src.to(buf.device, torch.float32))
            buf.mul_(scale)
            with trace_scope("fedavg_reduce"):
                dist.reduce(buf, dst=0, op=dist.ReduceOp.SUM)
            with trace_scope("fedavg_broadcast"):
                dist.broadcast(buf, src=0)
            src.copy_(buf.to(flat.device, flat.dtype))
        return weights

    def _reduce_buf(self, numel: int) -> torch.Tensor:
        coll_dev = self._coll_device()
        key = (numel, str(coll_dev))
        if key not in self._reduce_bufs:
            self._reduce_bufs[key] = torch.empty(
                numel, dtype=torch.float32, device=coll_dev
            )
        return self._reduce_bufs[key]

    def _fedavg_gpu_pipelined(self, src: torch.Tensor, buf: torch.Tensor,
                              scale: float) -> None:
        """Bucketed scale -> reduce -> broadcast -> cast-back, enqueued on
        the CALLER's current stream (the side stream in overlap mode).

        Overlap structure: the fused HIP scale_cast of bucket i+1 runs on
        this stream while RCCL moves bucket i on the communicator's own
        stream (async_op=True); the cast-back of bucket i overlaps the
        collectives of buckets > i. RCCL executes r0,b0,r1,b1,... in issue
        order, so each broadcast reads its completed reduce without any
        extra fencing (reference semantics: manager.py:119-126)."""
        from baton_amd.ops._ext import require_hip

        ops = require_hip()
        n = src.numel()
        bcast_works = []
        bounds = list(range(0, n, _BUCKET_ELEMS))
        with trace_scope("fedavg_reduce_bcast"):
            for off in bounds:
                end = min(off + _BUCKET_ELEMS, n)
                piece = buf[off:end]
                # pre-scale: buf = (n_i / N) * theta_i — fused HIP kernel
                ops.scale_cast(piece, src[off:end], scale)
                dist.reduce(piece, dst=0, op=dist.ReduceOp.SUM, async_op=True)
                bcast_works.append(
                    dist.broadcast(piece, src=0, async_op=True)
                )
            for off, w in zip(bounds, bcast_works):
                end = min(off + _BUCKET_ELEMS, n)
                w.wait()  # stream-level fence only (no host sync)
                ops.cast_copy(src[off:end], buf[off:end])

    # -- hipGraph-captured aggregation ----------------------------------------

    def capture_aggregation(self, arena: FlatParamArena, n_samples: int):
        """hipGraph-capture the WHOLE per-round aggregation sequence (the
        manager-side round loop on the data plane): per-group bucketed
        scale -> RCCL reduce -> broadcast -> cast-back plus the integer-
        buffer broadcasts, replayed as one graph per round.

        Valid while every rank's sample count stays fixed (the FedAvg
        scale is baked into the captured scale_cast); ``fedavg_arena``
        checks the weights each round and falls back to eager when they
        change. Requires GPU + a non-gloo backend."""
        if self.device.type != "cuda" or dist.get_backend() == "gloo":
            return False
        weights = self.gather_weights(n_samples)
        total = float(weights.sum().item())
        scale = float(n_samples) / total
        heaviest = int(torch.argmax(weights).item())
        int_bufs = [
            b for _, b in arena.model.named_buffers() if not b.is_floating_point()
        ]

        def _sequence():
            stream = self._side_stream or torch.cuda.current_stream()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                stream.wait_event(ev)
                for g in arena.all_groups:
                    src = g.flat.reshape(-1)
                    self._fedavg_gpu_pipelined(
                        src, self._reduce_buf(src.numel()), scale
                    )
                for b in int_bufs:
                    dist.broadcast(b.detach(), src=heaviest)
                done = torch.cuda.Event()
                done.record(stream)
            torch.cuda.current_stream().wait_event(done)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                _sequence()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _sequence()
        self._agg_graph = (graph, weights.clone(), float(n_samples))
        log.info("aggregation hipGraph captured (%d groups, %d int buffers)",
                 len(arena.all_groups), len(int_bufs))
        return True

    def fedavg_arena(
        self, arena: FlatParamArena, n_samples: int, async_handle: bool = False
    ) -> torch.Tensor:
        """FedAvg the whole model held in a FlatParamArena: params + float
        buffers averaged (one bucketed pipeline per dtype group); integer
        buffers broadcast from the heaviest client (same policy as
        fed.aggregate.fedavg_).

        async_handle=True (GPU overlap mode only) skips the final fence and
        returns a :class:`PendingAggregation` via ``self.pending``; the
        caller overlaps parameter-independent work with the collectives and
        calls ``pending.wait()`` before the first read of the averaged
        model. The returned value is always the weight vector."""
        weights = self.gather_weights(n_samples)
        total = float(weights.sum().item())
        if total <= 0:
            raise ValueError("total sample weight must be positive")
        if self._agg_graph is not None:
            graph, wcap, ncap = self._agg_graph
            if float(n_samples) == ncap and torch.equal(weights, wcap):
                graph.replay()
                # the captured sequence ends with the compute-stream fence
                self.pending = PendingAggregation(weights)
                return weights
            log.warning("sample weights changed — aggregation graph dropped")
            self._agg_graph = None
        scale = float(n_samples) / total
        heaviest = int(torch.argmax(weights).item())
        int_bufs = [
            b for _, b in arena.model.named_buffers() if not b.is_floating_point()
        ]
        self.pending = PendingAggregation(weights)  # pre-fenced default

        on_gpu = (
            self.device.type == "cuda"
            and dist.get_backend() != "gloo"
            and all(g.flat.device == self.device for g in arena.all_groups)
        )
        if on_gpu and self._side_stream is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(self._side_stream):
                self._side_stream.wait_event(ev)
                for g in arena.all_groups:
                    src = g.flat.reshape(-1)
                    self._fedavg_gpu_pipelined(
                        src, self._reduce_buf(src.numel()), scale
                    )
                for b in int_bufs:
                    dist.broadcast(b.detach(), src=heaviest)
                done = torch.cuda.Event()
                done.record(self._side_stream)
            self.pending = PendingAggregation(weights, done)
            if not async_handle:
                self.pending.wait()
            return weights

        for g in arena.all_groups:
            self.fedavg_flat(g.flat, n_samples, weights=weights)
        # integer buffers: copy from the heaviest rank (deterministic
        # tie-break: lowest rank wins, matching fed.aggregate)
        for b in int_bufs:
            t = b.detach()
            if dist.get_backend() == "gloo" and t.device.type != "cpu":
                cpu = t.cpu()
                dist.broadcast(cpu, src=heaviest)
                t.copy_(cpu)
            else:
                dist.broadcast(t, src=heaviest)
        return weights

    # -- server optimizer over clipped client updates ---------------------------

    def _arena_on_gpu(self, arena: FlatParamArena) -> bool:
        return (
            self.device.type == "cuda"
            and dist.get_backend() != "gloo"
            and all(g.flat.device == self.device for g in arena.all_groups)
        )

    def enable_server_opt(self, arena: FlatParamArena, cfg) -> None:
        """Allocate the state of ``fedopt_arena`` for ``arena`` (a collective:
        every rank calls it). Per dtype group: the fp32 master ``x`` and an
        fp32 reduce buffer on every rank, ``m`` and ``v`` on rank 0 only;
        once: ``partials``, ``clip_state``, ``w_slot``, ``round_state``.
        ``x`` is initialised from the arena and broadcast from rank 0, so
        all ranks start equal. Nothing is allocated per round. ``cfg`` is a
        ServerOptConfig with a name other than 'none'.

        With ``cfg.aggregator`` 'trimmed_mean' or 'median' (K = world size):
        ``flags`` [K], ``agg_state`` [k, b] and the int32 ``b_table`` [K + 1]
        on every rank, and on the GPU path, on rank 0 only, two fp32 staging
        buffers of K rows of one bucket (at most ``_BUCKET_ELEMS`` elements)
        that the clients' pieces are gathered into: 16 MiB per row, so 256 MB
        each at K = 16. World sizes above 16 are refused on the GPU path."""
        from baton_amd.fed import server_opt as so

        dp_z = float(getattr(cfg, "dp_noise_multiplier", 0.0))
        dp_seed = getattr(cfg, "dp_seed", None)
        dp_delta = float(getattr(cfg, "dp_delta", 1e-5))
        agg = getattr(cfg, "aggregator", "mean")
        beta = float(getattr(cfg, "trim_fraction", 0.1))
        so.validate(cfg.name, cfg.lr, cfg.beta1, cfg.beta2, cfg.tau,
                    cfg.client_clip_norm, dp_z, dp_seed, dp_delta, agg, beta)
        if cfg.name == "none":
            raise ValueError("enable_server_opt: server_opt.name is 'none'")
        on_gpu = self._arena_on_gpu(arena)
        dev = self.device if on_gpu else torch.device("cpu")
        f32 = dict(dtype=torch.float32, device=dev)
        robust = None
        if agg != "mean":
            K = self.world_size
            if on_gpu and K > 16:
                raise ValueError(
                    f"enable_server_opt: aggregator {agg!r} supports at most "
                    f"16 ranks on the device, got {K}")
            table = so.trim_table(agg, beta, K)
            if table[K] == 0 and self.rank == 0:
                log.warning(
                    "aggregator %s trims nothing at world size %d (b = 0): "
                    "it is the unweighted mean of the clipped updates", agg, K)
            stage = None
            if on_gpu and self.rank == 0:
                width = min(_BUCKET_ELEMS, max(
                    (g.flat.numel() + 3) // 4 * 4 for g in arena.all_groups))
                stage = [torch.empty((K, width), **f32) for _ in range(2)]
            robust = dict(
                aggregator=agg, table=table,
                flags=torch.zeros(K, **f32),
                agg_state=torch.zeros(2, **f32),
                b_table=torch.tensor(table, dtype=torch.int32, device=dev),
                stage=stage,
            )
        groups = []
        n_blocks = 0
        for i, g in enumerate(arena.all_groups):
            n = g.flat.numel()
            x = g.flat.detach().reshape(-1).to(**f32).clone()
            dist.broadcast(x, src=0)
            mode = cfg.name if i < len(arena.groups) else so.MEAN
            m = v = None
            if self.rank == 0 and mode != so.MEAN:
                m = torch.zeros(n, **f32)
                if mode in so.ADAPTIVE:
                    v = torch.full((n,), so.f32(so.f32(cfg.tau) ** 2), **f32)
            groups.append(dict(mode=mode, x=x, buf=torch.empty(n, **f32),
                               m=m, v=v))
            if on_gpu:
                from baton_amd.ops._ext import require_hip

                n_blocks += require_hip().optim_grid(n)
        self._fedopt = dict(
            arena=arena,
            on_gpu=on_gpu,
            name=cfg.name,
            lr=so.f32(cfg.lr), b1=so.f32(cfg.beta1), b2=so.f32(cfg.beta2),
            tau=so.f32(cfg.tau),
            clip=float(cfg.client_clip_norm) if cfg.client_clip_norm > 0
            else float("inf"),
            groups=groups,
            partials=torch.zeros(max(n_blocks, 1), **f32),
            clip_state=torch.zeros(4, **f32),
            w_slot=torch.zeros(1, **f32),
            round_state=torch.zeros(4, **f32),
            # DP-FedAvg (fed/server_opt.py): off with dp_z == 0. Only rank
            # 0's seed is ever used; dp_rounds counts every fedopt_arena call.
            dp_z=dp_z,
            dp_seed=so.resolve_seed(dp_seed) if dp_z > 0 else None,
            dp_delta=dp_delta,
            dp_rounds=0,
            # median / trimmed mean (fed/server_opt.py): None with 'mean'
            robust=robust,
        )

    @property
    def server_opt_enabled(self) -> bool:
        return self._fedopt is not None

    @property
    def fedopt_clip_state(self) -> torch.Tensor:
        """This rank's [norm, coef, finite, non-finite rounds so far]."""
        return self._fedopt["clip_state"]

    @property
    def fedopt_round_state(self) -> torch.Tensor:
        """[W, 1 / W or 0, applied 1 / 0, skipped rounds], equal on all ranks."""
        return self._fedopt["round_state"]

    @property
    def fedopt_agg_state(self) -> Optional[torch.Tensor]:
        """[k live clients, b trimmed per end] of the last round on rank 0;
        None with the 'mean' aggregator."""
        robust = self._fedopt["robust"]
        return None if robust is None else robust["agg_state"]

    @property
    def dp_enabled(self) -> bool:
        return self._fedopt is not None and self._fedopt["dp_z"] > 0

    @property
    def dp_rounds(self) -> int:
        """Rounds that drew noise so far (skipped rounds included)."""
        return self._fedopt["dp_rounds"]

    @property
    def dp_delta(self) -> float:
        return self._fedopt["dp_delta"]

    @property
    def dp_epsilon(self) -> float:
        """eps(dp_delta) spent so far (fed.server_opt.privacy_spent)."""
        from baton_amd.fed.server_opt import privacy_spent

        st = self._fedopt
        if st["dp_z"] <= 0:
            return 0.0
        return privacy_spent(st["dp_rounds"], st["dp_z"], st["dp_delta"])

    def server_opt_state(self) -> "dict[str, torch.Tensor]":
        """CPU copies of this rank's state: ``x.<group>`` and ``round_state``
        everywhere, ``m.<group>`` / ``v.<group>`` on rank 0; with DP noise on,
        the 0-dim int64 ``dp_rounds`` (never the seed)."""
        st = self._fedopt
        out = {"round_state": st["round_state"].detach().cpu().clone()}
        if st["dp_z"] > 0:
            out["dp_rounds"] = torch.tensor(st["dp_rounds"], dtype=torch.int64)
        for i, gs in enumerate(st["groups"]):
            for key in ("x", "m", "v"):
                if gs[key] is not None:
                    out[f"{key}.{i}"] = gs[key].detach().cpu().clone()
        return out

    def load_server_opt_state(self, state: "dict[str, torch.Tensor]") -> None:
        """Restore what ``server_opt_state`` returned on rank 0 (a collective:
        ``x`` and ``round_state`` are re-broadcast from rank 0, whose ``state``
        is the one that counts)."""
        st = self._fedopt
        if st["dp_z"] > 0 and "dp_rounds" in state:
            st["dp_rounds"] = int(state["dp_rounds"].item())
        if self.rank == 0:
            st["round_state"].copy_(state["round_state"])
        dist.broadcast(st["round_state"], src=0)
        for i, gs in enumerate(st["groups"]):
            if self.rank == 0:
                for key in ("x", "m", "v"):
                    if gs[key] is not None:
                        gs[key].copy_(state[f"{key}.{i}"])
            dist.broadcast(gs["x"], src=0)

    def _fedopt_gpu_sequence(self, arena: FlatParamArena, alpha: float,
                             dp: Optional[tuple] = None) -> None:
        """The device side of a round, enqueued on the CALLER's current
        stream. No host read: the clip coefficient, the participation and the
        skip decision stay in clip_state / w_slot / round_state.

          1. delta_sumsq per group, one clip_finalize
          2. delta_scale_cast of the first bucket, which writes w_slot
          3. reduce w_slot, fedopt_finalize on rank 0, broadcast round_state
          4. per bucket: delta_scale_cast, async reduce; on rank 0 wait()
             on that reduce (a stream fence) and server_step on the bucket;
             async broadcast of the x bucket; then cast_copy(theta, x)

        ``dp`` = (round t, sigma) turns the step into server_step_noise with
        (seed, t, group ordinal, the bucket's lo, sigma): buckets start at
        multiples of _BUCKET_ELEMS, so lo is a multiple of 4.

        Every reduce Work is kept and waited on, on every rank: nothing here
        relies on the communicator running reduce and broadcast of one
        buffer in issue order."""
        from baton_amd.ops._ext import require_hip

        ops = require_hip()
        st = self._fedopt
        root = self.rank == 0
        clip_state, w_slot, round_state = (
            st["clip_state"], st["w_slot"], st["round_state"])
        thetas = [g.flat.detach().reshape(-1) for g in arena.all_groups]
        with trace_scope("fedopt_norm"):
            off = 0
            for theta, gs in zip(thetas, st["groups"]):
                off += ops.delta_sumsq(theta, gs["x"], st["partials"], off)
            ops.clip_finalize(st["partials"], off, st["clip"], clip_state)
        buckets = [
            (gi, lo, min(lo + _BUCKET_ELEMS, theta.numel()))
            for gi, theta in enumerate(thetas)
            for lo in range(0, theta.numel(), _BUCKET_ELEMS)
        ]
        with trace_scope("fedopt_reduce_step_bcast"):
            gi, lo, hi = buckets[0]
            gs = st["groups"][gi]
            ops.delta_scale_cast(gs["buf"][lo:hi], thetas[gi][lo:hi],
                                 gs["x"][lo:hi], alpha, clip_state, w_slot)
            dist.reduce(w_slot, dst=0, op=dist.ReduceOp.SUM,
                        async_op=True).wait()
            if root:
                ops.fedopt_finalize(w_slot, round_state)
            dist.broadcast(round_state, src=0, async_op=True).wait()
            bcast_works = []
            for k, (gi, lo, hi) in enumerate(buckets):
                gs = st["groups"][gi]
                piece = gs["buf"][lo:hi]
                if k > 0:
                    ops.delta_scale_cast(piece, thetas[gi][lo:hi],
                                         gs["x"][lo:hi], alpha, clip_state,
                                         None)
                reduce_work = dist.reduce(piece, dst=0, op=dist.ReduceOp.SUM,
                                          async_op=True)
                reduce_work.wait()      # stream-level fence only
                if root:
                    step_args = (
                        gs["mode"], piece, gs["x"][lo:hi],
                        None if gs["m"] is None else gs["m"][lo:hi],
                        None if gs["v"] is None else gs["v"][lo:hi],
                        st["lr"], st["b1"], st["b2"], st["tau"], round_state)
                    if dp is None:
                        ops.server_step(*step_args)
                    else:
                        ops.server_step_noise(*step_args, st["dp_seed"],
                                              dp[0], gi, lo, dp[1])
                bcast_works.append(
                    dist.broadcast(gs["x"][lo:hi], src=0, async_op=True))
            for (gi, lo, hi), w in zip(buckets, bcast_works):
                w.wait()
                ops.cast_copy(thetas[gi][lo:hi], st["groups"][gi]["x"][lo:hi])

    def _fedopt_cpu_sequence(self, arena: FlatParamArena, alpha: float,
                             dp: Optional[tuple] = None) -> None:
        """The same round with torch ops (gloo / CPU): the arithmetic of
        fed.server_opt, the collectives of the device sequence; with ``dp``
        the noise is the oracle's (``dp_xi``)."""
        from baton_amd.fed import server_opt as so

        st = self._fedopt
        root = self.rank == 0
        cpu32 = dict(device="cpu", dtype=torch.float32)
        thetas = [g.flat.detach().reshape(-1) for g in arena.all_groups]
        deltas = [t.to(**cpu32) - gs["x"] for t, gs in zip(thetas, st["groups"])]
        sumsq = sum(float(d.double().pow(2).sum()) for d in deltas)
        norm, coef, finite = so.clip_coef(sumsq, st["clip"])
        cs = st["clip_state"]
        cs[0], cs[1], cs[2] = norm, coef, float(finite)
        if not finite:
            cs[3] += 1.0
        s = torch.tensor(alpha, dtype=torch.float32) * torch.tensor(
            coef, dtype=torch.float32)
        st["w_slot"][0] = alpha if finite else 0.0
        dist.reduce(st["w_slot"], dst=0, op=dist.ReduceOp.SUM)
        rs = st["round_state"]
        if root:
            W = st["w_slot"][0].item()
            inv_w, applied = so.inv_weight(W)
            rs[0], rs[1], rs[2] = W, inv_w, float(applied)
            if not applied:
                rs[3] += 1.0
        dist.broadcast(rs, src=0)
        for gi, (theta, d, gs) in enumerate(zip(thetas, deltas, st["groups"])):
            if finite:
                torch.mul(d, s, out=gs["buf"])
            else:
                gs["buf"].zero_()      # theta's NaN never meets the 0 weight
            dist.reduce(gs["buf"], dst=0, op=dist.ReduceOp.SUM)
            if root and rs[2].item() != 0.0:
                hp = (st["lr"], st["b1"], st["b2"], st["tau"])
                if dp is None:
                    so.server_update_(gs["mode"], gs["buf"], rs[1].item(),
                                      gs["x"], gs["m"], gs["v"], *hp)
                else:
                    xi = so.dp_xi(st["dp_seed"], dp[0], gi, 0,
                                  gs["buf"].numel(), dp[1])
                    so.server_apply_(gs["mode"], gs["buf"] + xi, gs["x"],
                                     gs["m"], gs["v"], *hp)
            dist.broadcast(gs["x"], src=0)
            theta.copy_(gs["x"].to(theta.dtype))

    def _robust_gpu_sequence(self, arena: FlatParamArena) -> None:
        """The device side of a round under 'trimmed_mean' or 'median', on
        the CALLER's current stream, without a host read:

          1. delta_sumsq per group, one clip_finalize (as the mean round)
          2. delta_scale_cast of the first bucket with alpha = 1.0: the
             piece is u_i = c_i d_i and w_slot the flag f_i
          3. gather w_slot into flags on rank 0, robust_finalize there,
             broadcast round_state
          4. per bucket: delta_scale_cast, async gather of the pieces into
             the rows of a staging buffer on rank 0, one bucket ahead of the
             step and alternating the two buffers
          5. on rank 0 wait() on that gather, robust_select of the staging
             rows into the reduce buffer's bucket, server_step on it
          6. async broadcast of the x bucket; then cast_copy(theta, x)

        Every gather and broadcast Work is kept and waited on, on every
        rank. A gather into a staging buffer is issued after the select that
        last read that buffer was enqueued, and collectives start behind the
        work already on the issuing stream."""
        from baton_amd.ops._ext import require_hip

        ops = require_hip()
        st = self._fedopt
        rb = st["robust"]
        root = self.rank == 0
        K = self.world_size
        clip_state, w_slot, round_state = (
            st["clip_state"], st["w_slot"], st["round_state"])
        flags, agg_state = rb["flags"], rb["agg_state"]
        thetas = [g.flat.detach().reshape(-1) for g in arena.all_groups]
        with trace_scope("fedopt_norm"):
            off = 0
            for theta, gs in zip(thetas, st["groups"]):
                off += ops.delta_sumsq(theta, gs["x"], st["partials"], off)
            ops.clip_finalize(st["partials"], off, st["clip"], clip_state)
        buckets = [
            (gi, lo, min(lo + _BUCKET_ELEMS, theta.numel()))
            for gi, theta in enumerate(thetas)
            for lo in range(0, theta.numel(), _BUCKET_ELEMS)
        ]

        def cast_and_gather(k: int, w_out):
            gi, lo, hi = buckets[k]
            gs = st["groups"][gi]
            piece = gs["buf"][lo:hi]
            ops.delta_scale_cast(piece, thetas[gi][lo:hi], gs["x"][lo:hi],
                                 1.0, clip_state, w_out)
            if w_out is not None:
                dist.gather(
                    w_slot, [flags[r:r + 1] for r in range(K)] if root
                    else None, dst=0, async_op=True).wait()
                if root:
                    ops.robust_finalize(flags, rb["b_table"], round_state,
                                        agg_state)
                dist.broadcast(round_state, src=0, async_op=True).wait()
            rows = None
            if root:
                stage = rb["stage"][k % 2]
                rows = [stage[r, :hi - lo] for r in range(K)]
            return dist.gather(piece, rows, dst=0, async_op=True)

        with trace_scope("fedopt_gather_select_step_bcast"):
            gather_work = cast_and_gather(0, w_slot)
            bcast_works = []
            for k, (gi, lo, hi) in enumerate(buckets):
                next_work = (cast_and_gather(k + 1, None)
                             if k + 1 < len(buckets) else None)
                gather_work.wait()      # stream-level fence only
                gs = st["groups"][gi]
                if root:
                    piece = gs["buf"][lo:hi]
                    ops.robust_select(piece, rb["stage"][k % 2][:, :hi - lo],
                                      flags, agg_state, round_state)
                    ops.server_step(
                        gs["mode"], piece, gs["x"][lo:hi],
                        None if gs["m"] is None else gs["m"][lo:hi],
                        None if gs["v"] is None else gs["v"][lo:hi],
                        st["lr"], st["b1"], st["b2"], st["tau"], round_state)
                bcast_works.append(
                    dist.broadcast(gs["x"][lo:hi], src=0, async_op=True))
                gather_work = next_work
            for (gi, lo, hi), w in zip(buckets, bcast_works):
                w.wait()
                ops.cast_copy(thetas[gi][lo:hi], st["groups"][gi]["x"][lo:hi])

    def _robust_cpu_sequence(self, arena: FlatParamArena) -> None:
        """The same round with torch ops (gloo / CPU): the collectives of the
        device sequence, the oracle helpers of fed.server_opt."""
        from baton_amd.fed import server_opt as so

        st = self._fedopt
        rb = st["robust"]
        root = self.rank == 0
        K = self.world_size
        cpu32 = dict(device="cpu", dtype=torch.float32)
        thetas = [g.flat.detach().reshape(-1) for g in arena.all_groups]
        deltas = [t.to(**cpu32) - gs["x"] for t, gs in zip(thetas, st["groups"])]
        sumsq = sum(float(d.double().pow(2).sum()) for d in deltas)
        norm, coef, finite = so.clip_coef(sumsq, st["clip"])
        cs = st["clip_state"]
        cs[0], cs[1], cs[2] = norm, coef, float(finite)
        if not finite:
            cs[3] += 1.0
        s = torch.tensor(1.0, dtype=torch.float32) * torch.tensor(
            coef, dtype=torch.float32)
        st["w_slot"][0] = 1.0 if finite else 0.0
        flags = rb["flags"]
        dist.gather(st["w_slot"],
                    [flags[r:r + 1] for r in range(K)] if root else None,
                    dst=0)
        rs = st["round_state"]
        live: list = []
        if root:
            live = [f != 0.0 for f in flags.tolist()]
            k, b, kept, inv, applied = so.robust_counts(live, rb["table"])
            rs[0], rs[1], rs[2] = float(kept), inv, float(applied)
            if not applied:
                rs[3] += 1.0
            rb["agg_state"][0], rb["agg_state"][1] = float(k), float(b)
        dist.broadcast(rs, src=0)
        for theta, d, gs in zip(thetas, deltas, st["groups"]):
            if finite:
                torch.mul(d, s, out=gs["buf"])
            else:
                gs["buf"].zero_()      # a dead row: gathered, never read
            rows = ([torch.empty_like(gs["buf"]) for _ in range(K)]
                    if root else None)
            dist.gather(gs["buf"], rows, dst=0)
            if root and rs[2].item() != 0.0:
                S = so.robust_sum(torch.stack(rows), live, rb["table"])
                so.server_update_(gs["mode"], S, rs[1].item(), gs["x"],
                                  gs["m"], gs["v"], st["lr"], st["b1"],
                                  st["b2"], st["tau"])
            dist.broadcast(gs["x"], src=0)
            theta.copy_(gs["x"].to(theta.dtype))

    def _fedopt_sequence(self, arena: FlatParamArena, alpha: float,
                         dp: Optional[tuple]) -> None:
        """The round's sequence for this plane's aggregator and device."""
        st = self._fedopt
        if st["robust"] is not None:
            if st["on_gpu"]:
                self._robust_gpu_sequence(arena)
            else:
                self._robust_cpu_sequence(arena)
        elif st["on_gpu"]:
            self._fedopt_gpu_sequence(arena, alpha, dp)
        else:
            self._fedopt_cpu_sequence(arena, alpha, dp)

    def fedopt_arena(
        self, arena: FlatParamArena, n_samples: int, async_handle: bool = False
    ) -> torch.Tensor:
        """One federated round through the server optimizer configured by
        ``enable_server_opt``: every rank sends its clipped update
        ``w_i c_i (theta_i - x)``, rank 0 steps the fp32 master ``x`` (and
        ``m``, ``v``), and every rank installs the broadcast ``x`` in its
        arena's dtype. A rank whose update is not finite sends zeros and
        weight 0; a round without any finite update leaves x, m and v as they
        were and still resets every rank to x. Integer buffers come from the
        heaviest client. The stream, side-stream and ``PendingAggregation``
        protocol is ``fedavg_arena``'s; the returned value is the weight
        vector. Under 'trimmed_mean' or 'median' the ranks send the unweighted
        ``c_i (theta_i - x)``, rank 0 gathers them and steps ``x`` with their
        coordinate-wise kept mean; ``n_samples`` then only picks the rank the
        integer buffers come from."""
        st = self._fedopt
        if st is None or st["arena"] is not arena:
            raise RuntimeError(
                "fedopt_arena: call enable_server_opt(arena, cfg) first")
        from baton_amd.fed.server_opt import dp_sigma, f32

        weights = self.gather_weights(n_samples)
        total = float(weights.sum().item())
        if total <= 0:
            raise ValueError("total sample weight must be positive")
        alpha = f32(float(n_samples) / total)
        dp = None
        if st["dp_z"] > 0:
            # the round index advances on every call, skipped rounds included
            dp = (st["dp_rounds"], dp_sigma(
                st["dp_z"], st["clip"],
                f32(float(weights.max().item()) / total)))
            st["dp_rounds"] += 1
        heaviest = int(torch.argmax(weights).item())
        int_bufs = [
            b for _, b in arena.model.named_buffers() if not b.is_floating_point()
        ]
        self.pending = PendingAggregation(weights)  # pre-fenced default

        if st["on_gpu"] and self._side_stream is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(self._side_stream):
                self._side_stream.wait_event(ev)
                self._fedopt_sequence(arena, alpha, dp)
                for b in int_bufs:
                    dist.broadcast(b.detach(), src=heaviest)
                done = torch.cuda.Event()
                done.record(self._side_stream)
            self.pending = PendingAggregation(weights, done)
            if not async_handle:
                self.pending.wait()
            return weights

        self._fedopt_sequence(arena, alpha, dp)
        for b in int_bufs:
            t = b.detach()
            if dist.get_backend() == "gloo" and t.device.type != "cpu":
                cpu = t.cpu()
                dist.broadcast(cpu, src=heaviest)
                t.copy_(cpu)
            else:
                dist.broadcast(t, src=heaviest)
        return weights

    def fedavg_model(self, model: torch.nn.Module, n_samples: int) -> torch.Tensor:
        """Arena-free path: average params + float buffers tensor-by-tensor
        (used for models that cannot be re-parented)."""
        weights = self.gather_weights(n_samples)
        named = [
            t
            for t in list(model.parameters()) + list(model.buffers())
            if t.is_floating_point()
        ]
        flat = torch.cat([t.detach().reshape(-1).float() for t in named])
        self.fedavg_flat(flat, n_samples, weights=weights)
        off = 0
        with torch.no_grad():
            for t in named:
                n = t.numel()
                t.copy_(flat[off : off + n].view(t.shape).to(t.dtype))
                off += n
        int_bufs = [b for b in model.buffers() if not b.is_floating_point()]
        if int_bufs:
            heaviest = int(torch.argmax(weights).item())
            for b in int_bufs:
                t = b.detach()
                if dist.get_backend() == "gloo" and t.device.type != "cpu":
                    cpu = t.cpu()
                    dist.broadcast(cpu, src=heaviest)
                    t.copy_(cpu)
                else:
                    dist.broadcast(t, src=heaviest)
        return weights

    # -- loss bookkeeping -------------------------------------------------------

    def weighted_mean_losses(
        self, loss_history: Sequence[float], weights: torch.Tensor
    ) -> List[float]:
        """Sample-weighted mean of per-epoch losses across ranks (the
        manager-side loss history of the HTTP path, manager.py:127-130).

        Histories may have unequal lengths across ranks (matching the HTTP
        path's weighted_loss_history): ranks agree on the max length first,
        zero-pad, and carry a per-epoch weight denominator so each epoch
        averages over exactly the ranks that reported it."""
        dev = self._coll_device()
        n = len(loss_history)
        ln = torch.tensor([float(n)], dtype=torch.float64, device=dev)
        dist.all_reduce(ln, op=dist.ReduceOp.MAX)
        length = int(ln.cpu().item())
        if length == 0:
            return []
        w = float(weights[self.rank].item())
        h = torch.zeros(2, length, dtype=torch.float64, device=dev)
        if n:
            h[0, :n] = torch.tensor(
                [float(x) for x in loss_history], dtype=torch.float64
            ).to(dev) * w
            h[1, :n] = w
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        num, den = h[0].cpu(), h[1].cpu()
        return [
            float(num[e] / den[e]) if float(den[e]) > 0 else float("nan")
            for e in range(length)
        ]

    def barrier(self) -> None:
        dist.barrier()

    @staticmethod
    def shutdown() -> None:
        if dist.is_initialized():
            dist.destroy_process_group()

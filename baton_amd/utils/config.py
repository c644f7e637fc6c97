"""Configuration for the whole engine.

The reference has no config system (SURVEY.md §5 "Config / flag system"):
three positional CLI args (demo.py:63-66) and keyword defaults scattered in
constructors (client_ttl=300 manager.py:22, heartbeat_time=60 / port=8080
worker.py:13-14, n_epoch=32 manager.py:53-55, lr=1e-3 / batch_size=32
demo.py:29). This module centralizes exactly those knobs — defaults preserved
— plus the MI355X additions (device, data plane, round deadline, checkpoint
dir), as one dataclass loadable from TOML.
"""

from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass, field
from typing import Optional


@dataclass
class ControlPlaneConfig:
    host: str = "127.0.0.1"
    port: int = 8080                 # reference worker.py:14 default
    client_ttl: float = 300.0        # reference manager.py:22
    cull_interval: Optional[float] = None   # default ttl/2, client_manager.py:23
    heartbeat_interval: float = 60.0        # reference worker.py:14
    # New (fixes defect D3/D7): rounds time out instead of hanging forever.
    round_deadline: Optional[float] = None  # seconds; None = no deadline
    # Partial-participation policy when the deadline fires or end_round is
    # forced: 'partial' aggregates responders (reference end_round semantics,
    # manager.py:118-126, made explicit), 'abort' discards the round.
    partial_policy: str = "partial"
    # Server-side aggregation mode. 'fedavg': the manager sample-weight-
    # averages the reported state_dicts (reference manager.py:119-126).
    # 'rccl': the clients already averaged over the xGMI data plane and the
    # manager COPIES rank 0's state_dict. This is a SERVER config switch on
    # purpose: a client-supplied "aggregated" flag must never be able to
    # flip the manager into copy mode (one client could then overwrite the
    # global model).
    aggregation_mode: str = "fedavg"

    @property
    def effective_cull_interval(self) -> float:
        return self.cull_interval if self.cull_interval is not None else self.client_ttl / 2


@dataclass
class TrainConfig:
    n_epoch: int = 32                # reference manager.py:55 default round length
    lr: float = 1e-3                 # reference demo.py:29
    batch_size: int = 32             # reference demo.py:29
    optimizer: str = "sgd"           # 'sgd' | 'adam' | 'adamw' (decoupled decay)
    momentum: float = 0.0
    weight_decay: float = 0.0
    max_grad_norm: float = 0.0       # >0 clips the global grad norm and skips
                                     # non-finite steps; 0 = off
    adam_betas: tuple = (0.9, 0.999)
    adam_eps: float = 1e-8
    fedprox_mu: float = 0.0          # >0 enables FedProx proximal term
    dtype: str = "float32"           # compute dtype: 'float32' | 'bfloat16'
    use_hip_graph: bool = False      # hipGraph-capture the local step
    progress: bool = False           # live tqdm epoch bar (reference
                                     # utils.py:70-90 parity); off when headless


@dataclass
class DataPlaneConfig:
    """RCCL-over-xGMI data plane (SURVEY.md §5 'Distributed communication')."""

    backend: str = "nccl"            # 'nccl' (=RCCL on ROCm) | 'gloo' (CPU tests)
    master_addr: str = "127.0.0.1"
    master_port: int = 29517
    # Overlap collectives with the next local step on a side HIP stream.
    overlap_stream: bool = True
    # Reduce dtype for the pre-scaled FedAvg reduce ('float32' is exact
    # enough to cross-check against the HTTP path bit-for-bit).
    reduce_dtype: str = "float32"


@dataclass
class ServerOptConfig:
    """Server-side step over clipped client updates (fed/server_opt.py)."""

    # 'none' (plain FedAvg, the code path without any of this) | 'fedavgm' |
    # 'fedadagrad' | 'fedadam' | 'fedyogi'
    name: str = "none"
    lr: float = 1.0
    beta1: float = 0.9
    beta2: float = 0.99
    tau: float = 1e-3                # adaptivity floor; v starts at tau^2
    client_clip_norm: float = 0.0    # >0 bounds each client's update norm;
                                     # 0 = off
    # DP-FedAvg: Gaussian noise of std z * client_clip_norm * max_i w_i on
    # the aggregate (fed/server_opt.py). 0 = off: every path stays as it is.
    dp_noise_multiplier: float = 0.0
    dp_seed: Optional[int] = None    # None = a fresh 64-bit seed per process
    dp_delta: float = 1e-5           # the delta of the reported epsilon
    # How the clients' updates become one Delta: 'mean' (the weighted sum, the
    # code path without any of this) | 'trimmed_mean' | 'median', coordinate-
    # wise over the clipped, unweighted updates (fed/server_opt.py).
    aggregator: str = "mean"
    trim_fraction: float = 0.1       # beta of 'trimmed_mean', in [0, 0.5)

    def __post_init__(self):
        from baton_amd.fed.server_opt import validate

        validate(self.name, self.lr, self.beta1, self.beta2, self.tau,
                 self.client_clip_norm, self.dp_noise_multiplier,
                 self.dp_seed, self.dp_delta, self.aggregator,
                 self.trim_fraction)

    @property
    def enabled(self) -> bool:
        return self.name != "none"


@dataclass
class BatonConfig:
    control: ControlPlaneConfig = field(default_factory=ControlPlaneConfig)
    train: TrainConfig = field(default_factory=TrainConfig)
    data_plane: DataPlaneConfig = field(default_factory=DataPlaneConfig)
    server_opt: ServerOptConfig = field(default_factory=ServerOptConfig)
    checkpoint_dir: Optional[str] = None   # persist global model per round
    device: str = "cuda"                   # 'cuda' (= ROCm HIP) | 'cpu'

    @classmethod
    def from_toml(cls, path: str) -> "BatonConfig":
        try:
            import tomllib  # py3.11+
        except ImportError:
            import tomli as tomllib
        with open(path, "rb") as f:
            raw = tomllib.load(f)
        return cls.from_dict(raw)

    @classmethod
    def from_dict(cls, raw: dict) -> "BatonConfig":
        def build(dc_cls, d):
            names = {f.name for f in dataclasses.fields(dc_cls)}
            kwargs = {}
            for k, v in d.items():
                if k not in names:
                    raise KeyError(f"unknown config key {dc_cls.__name__}.{k}")
                kwargs[k] = tuple(v) if isinstance(v, list) else v
            return dc_cls(**kwargs)

        cfg = cls()
        if "control" in raw:
            cfg.control = build(ControlPlaneConfig, raw["control"])
        if "train" in raw:
            cfg.train = build(TrainConfig, raw["train"])
        if "data_plane" in raw:
            cfg.data_plane = build(DataPlaneConfig, raw["data_plane"])
        if "server_opt" in raw:
            cfg.server_opt = build(ServerOptConfig, raw["server_opt"])
        for k in ("checkpoint_dir", "device"):
            if k in raw:
                setattr(cfg, k, raw[k])
        return cfg

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)


def local_rank() -> int:
    return int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))

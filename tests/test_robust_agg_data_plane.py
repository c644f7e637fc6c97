"""``fedopt_arena`` under the robust aggregators.

gloo at world 3 on the CPU: in round 0 rank 1 holds an update scaled by 1e6
and rank 2 a NaN. Rank 0 saves the server state before and after every round
and every rank what it sent and installed. The parent replays each round with
``ServerOptimizer`` (same config) from the stored state: the plane runs the
oracle's own helpers on the same numbers, so x, m and v agree by value.

RCCL at world 1 on the GPU (K = 1, Delta = u_0) against the oracle under the
bound of the world-1 test of tests/test_fedopt_exact.py, and ``"mean"`` against
a run without the new keys, bit for bit."""

from __future__ import annotations

import math
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fedopt_data_plane import _free_port, build_client_model  # noqa: E402
from test_fedopt_exact import (  # noqa: E402
    COEF_BOUND, E, HP, chain_of, native_ops, norm_bound, same_bits, step_ref,
    worst_ratio)

from baton_amd.fed.server_opt import ServerOptimizer  # noqa: E402

N_SAMPLES = {0: 96, 1: 288, 2: 64}       # rank 1, the scaled one, is heaviest
ROUNDS = 2
BAD_ROUND, SCALED_RANK, NAN_RANK = 0, 1, 2
CLIP = 0.0                               # off: the scaled update arrives whole


def _config(name: str, aggregator: str, **kw):
    from baton_amd.utils.config import ServerOptConfig

    return ServerOptConfig(
        name=name, lr=HP["lr"], beta1=HP["b1"], beta2=HP["b2"], tau=HP["tau"],
        client_clip_norm=CLIP, aggregator=aggregator, trim_fraction=0.34, **kw)


def _worker(rank: int, world: int, port: int, name: str, aggregator: str,
            out_dir: str):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig

    plane = FederatedDataPlane(DataPlaneConfig(backend="gloo", master_port=port),
                               device=torch.device("cpu"))
    model = build_client_model(rank)
    arena = FlatParamArena(model)
    plane.enable_server_opt(arena, _config(name, aggregator))
    assert plane.fedopt_agg_state is not None
    log = []
    for rnd in range(ROUNDS):
        gen = torch.Generator().manual_seed(10 * rnd + rank)
        scale = 1e6 if (rnd, rank) == (BAD_ROUND, SCALED_RANK) else 1.0
        for g in arena.all_groups:          # the client's local training
            g.flat.add_(scale * 0.1 * torch.randn(g.flat.numel(),
                                                  generator=gen))
        if (rnd, rank) == (BAD_ROUND, NAN_RANK):
            with torch.no_grad():
                model[2].weight[1, 3] = math.nan
        rec = {"before": plane.server_opt_state(),
               "sent": [g.flat.detach().clone() for g in arena.all_groups]}
        plane.fedopt_arena(arena, N_SAMPLES[rank])
        rec["after"] = plane.server_opt_state()
        rec["installed"] = [g.flat.detach().clone() for g in arena.all_groups]
        rec["agg_state"] = plane.fedopt_agg_state.clone()
        log.append(rec)
    assert arena.check_views()
    torch.save(log, os.path.join(out_dir, f"rank{rank}.pt"))
    plane.barrier()
    plane.shutdown()


@pytest.mark.parametrize("name,aggregator", [
    ("fedavgm", "median"), ("fedadam", "trimmed_mean")])
def test_gloo_world3_matches_the_cpu_oracle(tmp_path, name, aggregator):
    world = 3
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [
        ctx.Process(target=_worker,
                    args=(r, world, port, name, aggregator, str(tmp_path)))
        for r in range(world)
    ]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0, f"worker failed with {p.exitcode}"
    logs = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True)
            for r in range(world)]

    names = ["g0", "g1"]                      # the parameter and buffer groups
    oracle = ServerOptimizer.from_config(_config(name, aggregator))
    weights = [N_SAMPLES[r] for r in range(world)]
    for rnd in range(ROUNDS):
        before, after = logs[0][rnd]["before"], logs[0][rnd]["after"]
        for i, k in enumerate(names):
            oracle.x[k] = before[f"x.{i}"].clone()
        oracle.m["g0"] = before["m.0"].clone()
        if name == "fedadam":
            oracle.v["g0"] = before["v.0"].clone()
        clients = [OrderedDict(zip(names, log[rnd]["sent"])) for log in logs]
        global_sd = OrderedDict((k, t.clone()) for k, t in clients[0].items())
        oracle.step_(global_sd, clients, weights, ["g0"])
        bad = rnd == BAD_ROUND
        assert oracle.finite == [True, True, not bad]
        # k = 2 trims nothing; k = 3 drops one value at each end
        k, b = (2, 0) if bad else (3, 1)
        assert (oracle.last_live, oracle.last_trimmed) == (k, b)
        assert logs[0][rnd]["agg_state"].tolist() == [float(k), float(b)]
        kept = k - 2 * b
        assert after["round_state"].tolist() == [
            float(kept), float(np.float32(1.0 / kept)), 1.0, 0.0]
        for i, key in enumerate(names):
            assert torch.equal(after[f"x.{i}"], oracle.x[key]), (rnd, key)
            for log in logs:                  # every rank installs x
                assert torch.equal(log[rnd]["installed"][i], after[f"x.{i}"])
                assert torch.equal(log[rnd]["after"][f"x.{i}"],
                                   after[f"x.{i}"])
        assert torch.equal(after["m.0"], oracle.m["g0"])
        if name == "fedadam":
            assert torch.equal(after["v.0"], oracle.v["g0"])


# ---- "mean" keeps its bits -----------------------------------------------------------

def _mean_worker(rank: int, world: int, port: int, with_keys: bool,
                 out_dir: str):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    plane = FederatedDataPlane(DataPlaneConfig(backend="gloo", master_port=port),
                               device=torch.device("cpu"))
    arena = FlatParamArena(build_client_model(rank))
    kw = dict(aggregator="mean", trim_fraction=0.3) if with_keys else {}
    plane.enable_server_opt(arena, ServerOptConfig(
        name="fedadam", lr=HP["lr"], beta1=HP["b1"], beta2=HP["b2"],
        tau=HP["tau"], client_clip_norm=0.5, **kw))
    assert plane.fedopt_agg_state is None
    for rnd in range(2):
        gen = torch.Generator().manual_seed(10 * rnd + rank)
        for g in arena.all_groups:
            g.flat.add_(0.1 * torch.randn(g.flat.numel(), generator=gen))
        plane.fedopt_arena(arena, N_SAMPLES[rank])
    if rank == 0:
        torch.save(plane.server_opt_state(),
                   os.path.join(out_dir, f"mean{int(with_keys)}.pt"))
    plane.barrier()
    plane.shutdown()


def test_mean_gives_the_bits_of_a_run_without_the_keys(tmp_path):
    states = []
    for with_keys in (False, True):
        port = _free_port()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_mean_worker,
                             args=(r, 2, port, with_keys, str(tmp_path)))
                 for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
            assert p.exitcode == 0, f"worker failed with {p.exitcode}"
        states.append(torch.load(tmp_path / f"mean{int(with_keys)}.pt",
                                 weights_only=True))
    a, b = states
    assert list(a) == list(b)
    for k in a:
        assert same_bits(a[k], b[k]), k


# ---- RCCL, world 1 -------------------------------------------------------------------

def _nccl_world1_main():
    """Runs in a fresh process (see test_nccl_world1_robust)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29917",
                      RANK="0", WORLD_SIZE="1")
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    native_ops()
    plane = FederatedDataPlane(DataPlaneConfig(backend="nccl"),
                               device=torch.device("cuda", 0))
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(64, 128), nn.BatchNorm1d(128),
                          nn.Linear(128, 32)).to("cuda").bfloat16()
    model.train()
    model(torch.randn(8, 64, device="cuda").bfloat16())
    arena = FlatParamArena(model)
    names = [f"g{i}" for i in range(len(arena.all_groups))]
    cfg = ServerOptConfig(name="fedadam", lr=HP["lr"], beta1=HP["b1"],
                          beta2=HP["b2"], tau=HP["tau"], client_clip_norm=1.0,
                          aggregator="median")
    plane.enable_server_opt(arena, cfg)
    stage = plane._fedopt["robust"]["stage"]
    assert len(stage) == 2 and stage[0].shape[0] == 1
    assert stage[0].shape[1] % 4 == 0
    oracle = ServerOptimizer.from_config(cfg)
    flats = lambda: OrderedDict(
        (k, g.flat.detach().cpu().clone())
        for k, g in zip(names, arena.all_groups))
    T = max(chain_of(g.flat.numel(), 8) for g in arena.all_groups)
    rD = E + 2 * (E + COEF_BOUND + norm_bound(T))
    n_param_groups = len(arena.groups)

    worst = 0.0
    for rnd in range(2):
        gen = torch.Generator().manual_seed(50 + rnd)
        for g in arena.all_groups:              # the client's local training
            noise = 0.05 * torch.randn(g.flat.numel(), generator=gen)
            g.flat.add_(noise.to(g.flat.device, g.flat.dtype))
        before = plane.server_opt_state()
        client = flats()
        for i, k in enumerate(names):
            oracle.x[k] = before[f"x.{i}"].clone()
            if f"m.{i}" in before:
                oracle.m[k] = before[f"m.{i}"].clone()
                oracle.v[k] = before[f"v.{i}"].clone()
        plane.fedopt_arena(arena, 123, async_handle=True)
        plane.pending.wait()
        torch.cuda.synchronize()
        after = plane.server_opt_state()
        global_sd = OrderedDict((k, t.clone()) for k, t in client.items())
        oracle.step_(global_sd, [client], [123.0], names[:n_param_groups])
        assert (oracle.last_live, oracle.last_trimmed) == (1, 0)
        cs = plane.fedopt_clip_state.tolist()
        assert cs[2] == 1.0 and cs[1] < 1.0, cs      # clipped
        assert after["round_state"].tolist() == [1.0, 1.0, 1.0, 0.0]
        assert plane.fedopt_agg_state.tolist() == [1.0, 0.0]
        for i, k in enumerate(names):
            mode = "fedadam" if i < n_param_groups else "mean"
            z = np.zeros(before[f"x.{i}"].numel(), np.float32)
            ins = [before.get(f"{s}.{i}") for s in "xmv"]
            ins = [z if a is None else a.numpy() for a in ins]
            out = {s: after[f"{s}.{i}"].numpy() for s in "xmv"
                   if f"{s}.{i}" in after}
            ref = step_ref(mode, oracle.last_D[k].reshape(-1).numpy(), 1.0,
                           *ins, rD=rD)
            for s in out:
                worst = max(worst, worst_ratio(out[s], *ref[s]))
            g = arena.all_groups[i]
            assert same_bits(g.flat.detach().cpu(),
                             after[f"x.{i}"].to(g.flat.dtype))
        print(f"round {rnd}: worst {worst:.3f} of the bound")
        assert worst <= 1.0

    # a poisoned round: k = 0, nothing is written, the skip is counted
    before = plane.server_opt_state()
    with torch.no_grad():
        model[0].weight[3, 5] = math.inf
    plane.fedopt_arena(arena, 123)
    torch.cuda.synchronize()
    after = plane.server_opt_state()
    assert after["round_state"].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert plane.fedopt_agg_state.tolist() == [0.0, 0.0]
    for k in before:
        if k != "round_state":
            assert same_bits(before[k], after[k]), k
    for i, g in enumerate(arena.all_groups):
        assert torch.isfinite(g.flat).all()
    plane.shutdown()
    print("ROBUST-NCCL-1RANK-OK")


@pytest.mark.gpu
def test_nccl_world1_robust():
    native_ops()
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here])
    code = "import test_robust_agg_data_plane as t; t._nccl_world1_main()"
    proc = subprocess.run([sys.executable, "-c", code], env=env,
                          capture_output=True, text=True, timeout=300)
    print(proc.stdout[-3000:])
    assert proc.returncode == 0, (
        f"nccl world-1 robust round failed:\n{proc.stdout[-2000:]}\n"
        f"{proc.stderr[-4000:]}")
    assert "ROBUST-NCCL-1RANK-OK" in proc.stdout

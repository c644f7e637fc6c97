"""``fedopt_arena`` over gloo at world 2 on the CPU, against
``ServerOptimizer.step_``.

Two ranks with unequal sample counts run three rounds; in the second one rank
1's model holds a NaN. Rank 0 saves the server state before and after every
round and both ranks save what they sent and what they installed. The parent
replays each round with the oracle from the STORED state and holds the
plane's x, m and v to the bounds of tests/test_fedopt_exact.py (its
``step_ref``: float64 from the oracle's reduced D, rD = e: with two ranks the
reduce adds the same two numbers the oracle adds, so D itself is the same).
Both ranks must install bit-identical models, namely x in the model's dtype,
and integer buffers come from the heaviest rank."""

from __future__ import annotations

import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fedopt_exact import E, HP, step_ref, worst_ratio  # noqa: E402

from baton_amd.fed.server_opt import ServerOptimizer  # noqa: E402

N_SAMPLES = {0: 96, 1: 288}          # rank 1 is the heaviest client
ROUNDS = 3
NAN_ROUND, NAN_RANK = 1, 1
CLIP = 0.5


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def build_client_model(rank: int) -> nn.Module:
    """Per-rank model with BatchNorm (int + float buffers); the ranks differ,
    so enable_server_opt's broadcast of x from rank 0 shows."""
    torch.manual_seed(100 + rank)
    m = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8), nn.Linear(8, 2))
    m.train()
    for _ in range(rank + 1):
        m(torch.randn(8, 6))
    return m


def _worker(rank: int, world: int, port: int, name: str, out_dir: str):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    plane = FederatedDataPlane(DataPlaneConfig(backend="gloo", master_port=port),
                               device=torch.device("cpu"))
    model = build_client_model(rank)
    arena = FlatParamArena(model)
    assert not plane.server_opt_enabled
    with pytest.raises(RuntimeError, match="enable_server_opt"):
        plane.fedopt_arena(arena, N_SAMPLES[rank])
    plane.enable_server_opt(arena, ServerOptConfig(
        name=name, lr=HP["lr"], beta1=HP["b1"], beta2=HP["b2"], tau=HP["tau"],
        client_clip_norm=CLIP))
    assert plane.server_opt_enabled
    log = []
    for rnd in range(ROUNDS):
        gen = torch.Generator().manual_seed(10 * rnd + rank)
        for g in arena.all_groups:          # the client's local training
            g.flat.add_(0.1 * (rank + 1) * torch.randn(g.flat.numel(),
                                                       generator=gen))
        if (rnd, rank) == (NAN_ROUND, NAN_RANK):
            with torch.no_grad():
                model[2].weight[1, 3] = math.nan
        rec = {"before": plane.server_opt_state(),
               "sent": [g.flat.detach().clone() for g in arena.all_groups],
               "int_sent": model[1].num_batches_tracked.clone()}
        weights = plane.fedopt_arena(arena, N_SAMPLES[rank])
        assert weights.tolist() == [96.0, 288.0]
        assert plane.pending.wait() is weights
        rec["after"] = plane.server_opt_state()
        rec["installed"] = [g.flat.detach().clone() for g in arena.all_groups]
        rec["int_installed"] = model[1].num_batches_tracked.clone()
        rec["clip_state"] = plane.fedopt_clip_state.clone()
        log.append(rec)
    assert arena.check_views()
    # a restored state continues where the saved one stood (a collective)
    saved = plane.server_opt_state()
    for gs in plane._fedopt["groups"]:
        gs["x"].zero_()
    plane.load_server_opt_state(saved)
    again = plane.server_opt_state()
    assert all(torch.equal(saved[k], again[k]) for k in saved)
    torch.save(log, os.path.join(out_dir, f"rank{rank}.pt"))
    plane.barrier()
    plane.shutdown()


@pytest.mark.parametrize("name", ["fedavgm", "fedadam"])
def test_gloo_fedopt_matches_the_cpu_oracle(tmp_path, name):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [
        ctx.Process(target=_worker, args=(r, world, port, name, str(tmp_path)))
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
    oracle = ServerOptimizer(name, HP["lr"], HP["b1"], HP["b2"], HP["tau"],
                             CLIP)
    weights = [N_SAMPLES[r] for r in range(world)]
    tau2 = np.float32(np.float32(HP["tau"]) ** 2)
    worst = 0.0
    for rnd in range(ROUNDS):
        r0, r1 = logs[0][rnd], logs[1][rnd]
        before, after = r0["before"], r0["after"]
        if rnd == 0:
            # x is rank 0's model on both ranks; m = 0, v = tau^2 on rank 0
            x_init = torch.cat([
                t.detach().reshape(-1)
                for t in build_client_model(0).parameters()])
            assert torch.equal(before["x.0"], x_init)
            assert torch.equal(r1["before"]["x.0"], x_init)
            assert not before["m.0"].any()
            if name == "fedadam":
                assert (before["v.0"] == float(tau2)).all()
            else:
                assert "v.0" not in before
            assert "m.1" not in before and "m.0" not in r1["before"]
        for i, k in enumerate(names):
            oracle.x[k] = before[f"x.{i}"].clone()
            assert torch.equal(r1["before"][f"x.{i}"], before[f"x.{i}"])
        oracle.m["g0"] = before["m.0"].clone()
        if name == "fedadam":
            oracle.v["g0"] = before["v.0"].clone()
        clients = [OrderedDict(zip(names, log[rnd]["sent"])) for log in logs]
        global_sd = OrderedDict((k, t.clone()) for k, t in clients[0].items())
        oracle.step_(global_sd, clients, weights, ["g0"])
        nan_round = rnd == NAN_ROUND
        assert oracle.finite == [True, not nan_round]
        w0 = float(np.float32(96 / 384))
        want_w = w0 if nan_round else w0 + float(np.float32(288 / 384))
        assert after["round_state"].tolist() == [
            want_w, float(np.float32(1.0 / want_w)), 1.0, 0.0]
        for rank, log in enumerate(logs):
            cs = log[rnd]["clip_state"].tolist()
            assert cs[1] == oracle.coef[rank] < 1.0 or nan_round and rank == 1
            assert cs[2] == float(oracle.finite[rank])
        for i, k in enumerate(names):
            mode = name if i == 0 else "mean"
            z = np.zeros(before[f"x.{i}"].numel(), np.float32)
            ins = [before.get(f"{s}.{i}") for s in "xmv"]
            ins = [z if a is None else a.numpy() for a in ins]
            ref = step_ref(mode, oracle.last_D[k].numpy(), oracle.last_inv_W,
                           *ins, rD=E)
            for s in ref:
                worst = max(worst, worst_ratio(after[f"{s}.{i}"].numpy(),
                                               *ref[s]))
            # both ranks install x, bit for bit, and hold the same x
            for log in logs:
                assert torch.equal(log[rnd]["installed"][i], after[f"x.{i}"])
                assert torch.isfinite(log[rnd]["installed"][i]).all()
            assert torch.equal(r1["after"][f"x.{i}"], after[f"x.{i}"])
        # integer buffers come from the heaviest rank
        for log in logs:
            assert torch.equal(log[rnd]["int_installed"], r1["int_sent"])
        assert not torch.equal(r0["int_sent"], r1["int_sent"]) or rnd > 0
    print(f"{name}: worst {worst:.3f} of the bound")
    assert worst <= 1.0

"""DP-FedAvg on the CPU: the Philox4x32-10 oracle, the unit normals and their
layout, the accounting, ``ServerOptimizer`` with noise, the configuration and
manager plumbing, and one gloo world-2 ``fedopt_arena`` run.

Everything that is compared for bits is recomputed here in straight lines
from ``philox4x32`` / ``unit_normals`` and the numpy step of
tests/test_fedopt_exact.py (``emu_server_step`` with inv_W = 1, which leaves
Delta = D + xi as it is), never from the code under test's own step."""

from __future__ import annotations

import asyncio
import json
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
from test_fedopt_exact import HP, emu_server_step, same_bits_np  # noqa: E402

from baton_amd.control.manager import Experiment  # noqa: E402
from baton_amd.fed import server_opt as so  # noqa: E402
from baton_amd.fed.server_opt import (  # noqa: E402
    ServerOptimizer, f32, philox4x32, privacy_spent, unit_normals,
)
from baton_amd.utils.config import BatonConfig, ServerOptConfig  # noqa: E402

SEED = 0x0123456789ABCDEF       # picked once; the statistics below are its
Z, CLIP, DELTA = 1.1, 0.5, 1e-5
RS_ONE = np.asarray([1.0, 1.0, 1.0, 0.0], np.float32)    # inv_W = 1


# ---- Philox ------------------------------------------------------------------

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = philox4x32(counter, key)
    assert " ".join(f"{int(w):08x}" for w in got) == want
    # vectorised over the counter: the same words at every position
    arr = philox4x32([np.full(3, c, np.uint64) for c in counter], key)
    assert all(w.dtype == np.uint32 and w.shape == (3,) for w in arr)
    assert " ".join(f"{int(w[2]):08x}" for w in arr) == want


def normals_of_block(seed, rnd, stream, j):
    """The four normals of block j, one scalar operation at a time."""
    r = [int(w) for w in philox4x32(
        (j & 0xFFFFFFFF, j >> 32, rnd & 0xFFFFFFFF, stream),
        (seed & 0xFFFFFFFF, seed >> 32))]
    out = []
    for a, b in ((r[0], r[1]), (r[2], r[3])):
        u1 = ((a >> 8) + 1) * 2.0 ** -24
        u2 = (b >> 8) * 2.0 ** -24
        R = math.sqrt(-2.0 * math.log(u1))
        out += [R * math.cos(2 * math.pi * u2), R * math.sin(2 * math.pi * u2)]
    return out


def test_unit_normals_layout():
    z = unit_normals(SEED, 3, 2, 0, 64)
    assert z.dtype == np.float64 and z.shape == (64,)
    for j in (0, 1, 7, 15):
        want = normals_of_block(SEED, 3, 2, j)
        # lane e & 3 of block e >> 2; the float64 trig differs from the
        # quadrant-reduced one by its own rounding only
        np.testing.assert_allclose(z[4 * j: 4 * j + 4], want, rtol=0,
                                   atol=1e-14)
    # an offset of 4 k is a slice of offset 0, and so is any other offset
    for off, n in ((4, 60), (16, 5), (20, 44), (3, 9), (62, 2)):
        assert np.array_equal(unit_normals(SEED, 3, 2, off, n),
                              z[off: off + n])
    assert unit_normals(SEED, 3, 2, 8, 0).shape == (0,)
    # the carry into hi32(j)
    off = 4 * (2 ** 32 - 1)
    far = unit_normals(SEED, 3, 2, off, 8)
    np.testing.assert_allclose(
        far, normals_of_block(SEED, 3, 2, 2 ** 32 - 1)
        + normals_of_block(SEED, 3, 2, 2 ** 32), rtol=0, atol=1e-14)
    assert not np.array_equal(far[4:], z[:4])               # j = 2^32 is not 0
    # streams, rounds and both halves of the seed each change the values
    for other in (unit_normals(SEED, 3, 3, 0, 64),
                  unit_normals(SEED, 4, 2, 0, 64),
                  unit_normals(SEED ^ 1, 3, 2, 0, 64),
                  unit_normals(SEED ^ (1 << 40), 3, 2, 0, 64)):
        assert not np.any(other == z)
    assert np.array_equal(unit_normals(SEED, 3, 2, 0, 64), z)
    # cospi's and sinpi's zeros are exact: u2 = 0, 1/4, 1/2, 3/4
    b = (np.asarray([0, 1, 2, 3], np.uint32) << np.uint32(30))
    a = np.full(4, 0x12345678, np.uint32)
    c, s = so._box_muller64(a, b)
    assert c[1] == 0.0 and c[3] == 0.0 and s[0] == 0.0 and s[2] == 0.0
    assert c[0] == -c[2] > 0 and s[1] == -s[3] > 0
    for bad in (dict(seed=-1), dict(seed=2 ** 64), dict(stream=2 ** 32),
                dict(stream=-1), dict(round=-1), dict(offset=-4), dict(n=-1)):
        kw = dict(seed=SEED, round=0, stream=0, offset=0, n=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            unit_normals(**kw)


def test_unit_normals_statistics():
    n = 1 << 20
    z = unit_normals(SEED, 0, 0, 0, n)
    mean, var = float(z.mean()), float(z.var())
    print(f"mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 "
          f"{var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e}), max |z| "
          f"{np.abs(z).max():.3f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert np.abs(z).max() <= math.sqrt(48 * math.log(2))


# ---- accounting ----------------------------------------------------------------

@pytest.mark.parametrize("T,z,delta", [(1, 1.0, 1e-5), (100, 1.1, 1e-5),
                                       (1000, 0.7, 1e-6), (37, 4.0, 1e-3)])
def test_privacy_spent(T, z, delta):
    got = privacy_spent(T, z, delta)
    assert isinstance(got, float)
    assert got == T / (2 * z * z) + math.sqrt(2 * T * math.log(1 / delta)) / z
    # the Renyi bound it is the closed-form optimum of, on a fine grid
    am1 = np.exp(np.linspace(math.log(1e-4), math.log(1e4), 2_000_001))
    grid = (1 + am1) * T / (2 * z * z) + math.log(1 / delta) / am1
    assert abs(grid.min() / got - 1) <= 1e-9
    assert grid.min() >= got * (1 - 1e-12)


def test_privacy_spent_edges():
    assert privacy_spent(0, 1.0, 1e-5) == 0.0
    assert privacy_spent(3, 0.0, 1e-5) == math.inf
    for bad in (0.0, 1.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            privacy_spent(3, 1.0, bad)


# ---- ServerOptimizer -------------------------------------------------------------

def make_model(seed):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8))
    m.train()
    m(torch.randn(8, 6))
    return m


def sd_of(model):
    return OrderedDict((k, v.detach().clone())
                       for k, v in model.state_dict().items())


def clients_for(global_sd, rnd, k=3, scale=0.05):
    out = []
    for i in range(k):
        gen = torch.Generator().manual_seed(1000 * rnd + i)
        sd = OrderedDict()
        for key, t in global_sd.items():
            if t.is_floating_point():
                sd[key] = t + scale * (i + 1) * torch.randn(t.shape,
                                                            generator=gen)
            else:
                sd[key] = t + i + rnd
        out.append(sd)
    return out


def bits_equal(a, b):
    if a.is_floating_point():
        return a.dtype == b.dtype and torch.equal(
            a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def optimizer(name="fedadam", **kw):
    return ServerOptimizer(name, HP["lr"], HP["b1"], HP["b2"], HP["tau"],
                           CLIP, **kw)


def expected_step(name, D, x0, m0, v0, seed, t, stream, offset, sigma):
    """x, m, v after one applied noised step, in numpy, from the stored
    inputs: xi = fl(sigma fl(zeta)), Delta = fl(D + xi), then the mode."""
    D = np.asarray(D, np.float32).reshape(-1)
    zeta = unit_normals(seed, t, stream, offset, D.size).astype(np.float32)
    delta = D + np.float32(sigma) * zeta
    z = np.zeros(D.size, np.float32)
    flat = lambda a: z if a is None else np.asarray(a, np.float32).reshape(-1)
    return emu_server_step(name, delta, flat(x0), flat(m0), flat(v0), RS_ONE)


WEIGHTS = [96, 288, 160]


@pytest.mark.parametrize("name", so.MODES)
def test_server_optimizer_with_noise_is_the_definition(name):
    model = make_model(0)
    gsd = sd_of(model)
    params = [n for n, _ in model.named_parameters()]
    fkeys = [k for k, t in gsd.items() if t.is_floating_point()]
    opt = optimizer(name, noise_multiplier=Z, seed=SEED)
    twin = optimizer(name)                     # no noise: the source of D
    assert opt.seed == SEED and opt.dp_rounds == 0
    sigma = f32(Z * CLIP * f32(288 / 544))
    skipped = 0
    for t in range(4):
        clients = clients_for(gsd, t)
        if t == 1:                             # a skipped round
            for sd in clients:
                sd["0.weight"][0, 0] = math.inf
        if t == 0:
            twin._ensure_state(gsd, params)
            opt._ensure_state(gsd, params)
        for d in ("x", "m", "v"):
            setattr(twin, d, OrderedDict(
                (k, a.clone()) for k, a in getattr(opt, d).items()))
        before = {d: {k: a.clone() for k, a in getattr(opt, d).items()}
                  for d in ("x", "m", "v")}
        twin.step_(OrderedDict((k, a.clone()) for k, a in gsd.items()),
                   clients, WEIGHTS, params)
        opt.step_(gsd, clients, WEIGHTS, params)
        assert opt.dp_rounds == t + 1          # applied or not
        if t == 1:
            skipped += 1
            assert not opt.applied
            for d in before:
                for k, a in before[d].items():
                    assert bits_equal(getattr(opt, d)[k], a)
            assert opt.skipped_rounds == skipped
            continue
        assert opt.applied and opt.last_sigma == sigma
        for s, k in enumerate(fkeys):
            mode = name if k in params else "mean"
            want = expected_step(mode, twin.last_D[k], before["x"][k],
                                 before["m"].get(k), before["v"].get(k),
                                 SEED, t, s, 0, sigma)
            assert same_bits_np(opt.x[k].numpy().reshape(-1), want["x"]), k
            if k in opt.m:
                assert same_bits_np(opt.m[k].numpy().reshape(-1), want["m"])
            if k in opt.v:
                assert same_bits_np(opt.v[k].numpy().reshape(-1), want["v"])
            # the noise is there, and the buffers take it too
            assert not bits_equal(opt.x[k], twin.x[k]), k
            assert bits_equal(gsd[k], opt.x[k].to(gsd[k].dtype))


def test_state_dict_carries_dp_rounds_and_never_the_seed():
    model = make_model(0)
    gsd = sd_of(model)
    params = [n for n, _ in model.named_parameters()]
    opt = optimizer(noise_multiplier=Z, seed=SEED)
    for t in range(2):
        opt.step_(gsd, clients_for(gsd, t), WEIGHTS, params)
    state = opt.state_dict()
    assert state["dp_rounds"].dtype == torch.int64
    assert state["dp_rounds"].dim() == 0 and int(state["dp_rounds"]) == 2
    for k, a in state.items():
        assert "seed" not in k
        assert not (a.dtype == torch.int64 and a.numel()
                    and int(a.reshape(-1)[0]) in (SEED, SEED - 2 ** 64))
    again = optimizer(noise_multiplier=Z, seed=SEED)
    again.load_state_dict(state)
    assert again.dp_rounds == 2
    gsd2 = OrderedDict((k, a.clone()) for k, a in gsd.items())
    clients = clients_for(gsd, 2)
    opt.step_(gsd, clients, WEIGHTS, params)
    again.step_(gsd2, clients, WEIGHTS, params)
    a, b = opt.state_dict(), again.state_dict()
    assert list(a) == list(b) and all(bits_equal(a[k], b[k]) for k in a)
    assert opt.epsilon == privacy_spent(3, Z, 1e-5)
    # a fresh seed per object when none is given
    s1 = optimizer(noise_multiplier=Z).seed
    s2 = optimizer(noise_multiplier=Z).seed
    assert s1 != s2 and 0 <= s1 < 2 ** 64


def test_zero_multiplier_changes_nothing():
    model = make_model(0)
    params = [n for n, _ in model.named_parameters()]
    g1, g2 = sd_of(model), sd_of(model)
    a = optimizer()
    b = optimizer(noise_multiplier=0.0, seed=SEED, delta=1e-5)
    for t in range(3):
        clients = clients_for(g1, t)
        a.step_(g1, clients, WEIGHTS, params)
        b.step_(g2, clients, WEIGHTS, params)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and "dp_rounds" not in sb
    assert all(bits_equal(sa[k], sb[k]) for k in sa)
    assert all(bits_equal(g1[k], g2[k]) for k in g1)
    assert b.dp_rounds == 0 and b.seed is None and b.epsilon == 0.0
    assert set(sb) == {"skipped_rounds"} | {
        f"{p}.{k}" for p, d in (("x", b.x), ("m", b.m), ("v", b.v))
        for k in d}


# ---- refusals and plumbing ---------------------------------------------------------

def test_refusals():
    ok = dict(name="fedadam", client_clip_norm=1.0, dp_noise_multiplier=1.0)
    ServerOptConfig(**ok)
    ServerOptConfig(**ok, dp_seed=0)
    ServerOptConfig(**ok, dp_seed=2 ** 64 - 1)
    bad = [dict(name="none"),
           dict(client_clip_norm=0.0), dict(client_clip_norm=math.inf),
           dict(dp_noise_multiplier=-1.0), dict(dp_noise_multiplier=math.inf),
           dict(dp_noise_multiplier=math.nan),
           dict(dp_delta=0.0), dict(dp_delta=1.0), dict(dp_delta=-0.1),
           dict(dp_delta=math.nan),
           dict(dp_seed=-1), dict(dp_seed=2 ** 64)]
    for kw in bad:
        kw = {**ok, **kw}
        with pytest.raises(ValueError):
            ServerOptConfig(**kw)
        with pytest.raises(ValueError):
            BatonConfig.from_dict({"server_opt": kw})
        if kw["name"] == "none":
            continue
        with pytest.raises(ValueError):
            ServerOptimizer(kw["name"], client_clip_norm=kw["client_clip_norm"],
                            noise_multiplier=kw["dp_noise_multiplier"],
                            seed=kw.get("dp_seed"),
                            delta=kw.get("dp_delta", 1e-5))
    # with z = 0 none of this is looked at: today's configurations stand
    ServerOptConfig(name="none")
    ServerOptConfig(name="fedadam", client_clip_norm=0.0)
    assert ServerOptConfig().dp_noise_multiplier == 0.0
    assert ServerOptConfig().dp_seed is None
    assert ServerOptConfig().dp_delta == 1e-5


def test_config_plumbing(tmp_path):
    raw = {"server_opt": {"name": "fedyogi", "client_clip_norm": 2.0,
                          "dp_noise_multiplier": 0.8, "dp_seed": SEED,
                          "dp_delta": 1e-6}}
    cfg = BatonConfig.from_dict(raw)
    assert (cfg.server_opt.dp_noise_multiplier, cfg.server_opt.dp_seed,
            cfg.server_opt.dp_delta) == (0.8, SEED, 1e-6)
    again = BatonConfig.from_dict(
        {k: v for k, v in cfg.to_dict().items() if v is not None})
    assert again.server_opt == cfg.server_opt
    path = tmp_path / "baton.toml"
    path.write_text('[server_opt]\nname = "fedadam"\nclient_clip_norm = 1.5\n'
                    "dp_noise_multiplier = 1.2\ndp_seed = 77\n"
                    "dp_delta = 1e-7\n")
    toml = BatonConfig.from_toml(str(path))
    assert toml.server_opt == ServerOptConfig(
        name="fedadam", client_clip_norm=1.5, dp_noise_multiplier=1.2,
        dp_seed=77, dp_delta=1e-7)
    opt = ServerOptimizer.from_config(toml.server_opt)
    assert (opt.noise_multiplier, opt.seed, opt.delta) == (1.2, 77, 1e-7)
    with pytest.raises(KeyError, match="ServerOptConfig.dp_sigma"):
        BatonConfig.from_dict({"server_opt": {"dp_sigma": 1.0}})
    # the launcher's flags
    from baton_amd.parallel import launcher

    src = open(launcher.__file__).read()
    for flag in ("--dp-noise-multiplier", "--dp-seed", "--dp-delta"):
        assert flag in src


def _run_round(exp, responses):
    exp.rounds.begin(set(responses))
    for cid in responses:
        exp.rounds.client_started(cid)
    for cid, rec in responses.items():
        exp.rounds.record(cid, rec)
    asyncio.run(exp.end_round(reason="complete"))


def _responses(clients, weights):
    return {
        f"c{i}": {"state_dict": sd, "n_samples": n, "loss_history": [1.0],
                  "aggregated": False}
        for i, (sd, n) in enumerate(zip(clients, weights))
    }


def _metrics(exp):
    return json.loads(asyncio.run(exp.handle_metrics(None)).body)


def test_manager_metrics_and_sidecar(tmp_path):
    cfg = BatonConfig(checkpoint_dir=str(tmp_path))
    cfg.server_opt = ServerOptConfig(
        name="fedadam", client_clip_norm=CLIP, dp_noise_multiplier=Z,
        dp_seed=SEED, dp_delta=DELTA, lr=HP["lr"], beta1=HP["b1"],
        beta2=HP["b2"], tau=HP["tau"])
    exp = Experiment(make_model(0), "exp", app=None, config=cfg)
    m0 = _metrics(exp)
    assert m0["dp_rounds"] == 0 and m0["dp_epsilon"] == 0.0
    for rnd in range(2):
        _run_round(exp, _responses(clients_for(sd_of(exp.model), rnd),
                                   WEIGHTS))
    m = _metrics(exp)
    assert m["dp_rounds"] == 2
    assert m["dp_epsilon"] == privacy_spent(2, Z, DELTA)
    assert not any("seed" in k for k in m)
    assert str(SEED) not in json.dumps(m)
    # the sidecar keeps dp_rounds and not the seed
    from baton_amd.control.wire import decode_payload

    blob = (tmp_path / "exp.server_opt.ckpt").read_bytes()
    meta, tensors = decode_payload(blob)
    assert int(tensors["dp_rounds"]) == 2
    assert not any("seed" in k for k in list(meta) + list(tensors))
    for word in (SEED.to_bytes(8, "little"), SEED.to_bytes(8, "big"),
                 str(SEED).encode()):
        assert word not in blob
    again = Experiment(make_model(7), "exp", app=None, config=cfg)
    assert again.load_checkpoint()
    assert again.server_opt.dp_rounds == 2
    assert _metrics(again)["dp_epsilon"] == m["dp_epsilon"]
    clients = clients_for(sd_of(exp.model), 2)
    _run_round(exp, _responses(clients, WEIGHTS))
    _run_round(again, _responses(clients, WEIGHTS))
    for k, t in exp.model.state_dict().items():
        assert bits_equal(t, again.model.state_dict()[k]), k
    assert _metrics(again)["dp_rounds"] == 3
    # without noise the metrics are what they were
    cfg.server_opt = ServerOptConfig(name="fedadam", client_clip_norm=CLIP)
    plain = Experiment(make_model(0), "plain", app=None, config=cfg)
    assert "dp_rounds" not in plain.metrics
    assert "dp_epsilon" not in plain.metrics


# ---- gloo, world 2 -----------------------------------------------------------------

N_SAMPLES = {0: 96, 1: 288}
ROUNDS = 2


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def build_client_model(rank: int) -> nn.Module:
    torch.manual_seed(100 + rank)
    m = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8), nn.Linear(8, 2))
    m.train()
    for _ in range(rank + 1):
        m(torch.randn(8, 6))
    return m


def _worker(rank: int, world: int, port: int, out_dir: str):
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
    # only rank 0's seed counts: rank 1 draws its own
    plane.enable_server_opt(arena, ServerOptConfig(
        name="fedadam", lr=HP["lr"], beta1=HP["b1"], beta2=HP["b2"],
        tau=HP["tau"], client_clip_norm=CLIP, dp_noise_multiplier=Z,
        dp_seed=SEED if rank == 0 else None, dp_delta=DELTA))
    assert plane.dp_enabled and plane.dp_rounds == 0
    log = []
    for rnd in range(ROUNDS):
        gen = torch.Generator().manual_seed(10 * rnd + rank)
        for g in arena.all_groups:
            g.flat.add_(0.1 * (rank + 1) * torch.randn(g.flat.numel(),
                                                       generator=gen))
        rec = {"before": plane.server_opt_state()}
        plane.fedopt_arena(arena, N_SAMPLES[rank])
        rec["after"] = plane.server_opt_state()
        rec["D"] = [gs["buf"].clone() for gs in plane._fedopt["groups"]]
        rec["installed"] = [g.flat.detach().clone() for g in arena.all_groups]
        log.append(rec)
        assert plane.dp_rounds == rnd + 1
        assert plane.dp_epsilon == privacy_spent(rnd + 1, Z, DELTA)
    saved = plane.server_opt_state()
    assert int(saved["dp_rounds"]) == ROUNDS and "dp_seed" not in saved
    plane._fedopt["dp_rounds"] = 0
    plane.load_server_opt_state(saved)
    assert plane.dp_rounds == ROUNDS
    torch.save(log, os.path.join(out_dir, f"rank{rank}.pt"))
    plane.barrier()
    plane.shutdown()


def test_gloo_fedopt_with_noise_for_bits(tmp_path):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path)))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0, f"worker failed with {p.exitcode}"
    logs = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True)
            for r in range(world)]
    sigma = f32(Z * CLIP * f32(288 / 384))
    for rnd in range(ROUNDS):
        r0, r1 = logs[0][rnd], logs[1][rnd]
        before, after = r0["before"], r0["after"]
        assert int(before["dp_rounds"]) == rnd
        assert int(after["dp_rounds"]) == rnd + 1
        assert after["round_state"].tolist()[2] == 1.0
        for gi, mode in enumerate(("fedadam", "mean")):
            want = expected_step(
                mode, r0["D"][gi], before[f"x.{gi}"], before.get(f"m.{gi}"),
                before.get(f"v.{gi}"), SEED, rnd, gi, 0, sigma)
            for s in "xmv":
                if f"{s}.{gi}" in after:
                    assert same_bits_np(after[f"{s}.{gi}"].numpy(), want[s]), (
                        rnd, gi, s)
            # a wrong stream or round is not the same step
            other = expected_step(
                mode, r0["D"][gi], before[f"x.{gi}"], before.get(f"m.{gi}"),
                before.get(f"v.{gi}"), SEED, rnd + 1, gi, 0, sigma)
            assert not same_bits_np(after[f"x.{gi}"].numpy(), other["x"])
            # both ranks install rank 0's x
            assert bits_equal(r1["after"][f"x.{gi}"], after[f"x.{gi}"])
            assert bits_equal(r0["installed"][gi], after[f"x.{gi}"])
            assert bits_equal(r1["installed"][gi], after[f"x.{gi}"])

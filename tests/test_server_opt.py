"""The server optimizers on the CPU (fed/server_opt.py, the manager's
``end_round`` and sidecar checkpoint, ``ServerOptConfig``).

``ServerOptimizer.step_`` is held against a float64 recomputation of each
round from the optimizer's STORED fp32 state (x, m, v before the round) and
the clients' stored tensors. With e = 2^-24 per fp32 operation and k clients,
the oracle's Delta = fl(fl(sum_i fl(fl(w_i c_i) fl(theta_i - x))) inv_W)
carries: the subtraction (e), the rounding of c_i to fp32 (e), the product
w_i c_i (e), the product with d_i (e), k additions (k e, the first onto 0.0
is exact), the k - 1 additions of W and the rounding of 1 / W (k e), and the
final product (e), each relative to A = sum_i |w_i c_i d_i| / W at most:

    dDelta = (5 + 2 k) e A

and then, operation by operation as in tests/test_fedopt_exact.py (whose
bounds these are, with Delta's error given absolutely), K = 1 + 2^-10:

    mean      dx = dDelta + e |x|
    fedavgm   dm = dDelta + e |m|,  dx = lr dm + e |x|
    adaptive  dm = (1 - b1)(dDelta + 2 e |Delta|) + e |m|
              dv = [2 |Delta| dDelta (+ 3 e Delta^2)] (1 - b2 or 1) + e v
                   (adagrad: no (1 - b2), no 3 e); Yogi adds 2 (1 - b2) Delta^2
                   where |v0 - Delta^2| <= 2 |Delta| dDelta + 2 e Delta^2
              rd = dv / (2 v) + 2 e,  dq = (dm + |m| (rd + e)) / denom
              dx = lr dq + e |x|

The oracle forms an fma as the float64 product and sum rounded to fp32; the
double rounding adds 2^-29 e, which K covers."""

import asyncio
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from baton_amd.control.manager import Experiment
from baton_amd.fed.aggregate import fedavg_
from baton_amd.fed.server_opt import MODES, ServerOptimizer, f32
from baton_amd.utils.config import BatonConfig, ServerOptConfig

E = 2.0 ** -24
K2 = 1.0 + 2.0 ** -10
HP = dict(lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)


def make_model(seed, steps=1):
    """Linear + BatchNorm1d with float and integer buffers that differ."""
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(6, 8), nn.BatchNorm1d(8))
    m.train()
    for _ in range(steps):
        m(torch.randn(8, 6))
    return m


def sd_of(model):
    return OrderedDict((k, v.detach().clone())
                       for k, v in model.state_dict().items())


def param_names(model):
    return [n for n, _ in model.named_parameters()]


def clients_for(global_sd, rnd, k=3, scale=0.05):
    """k client state dicts: the global model plus seeded noise."""
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


def round_ref(opt, key, is_param, x0, m0, v0, thetas, weights, clip):
    """{name: (float64 reference, bound)} for one key of one applied round.
    Norms are over all float keys, so the coefficients come in via ``clip``
    = the list of float64 coefficients."""
    total = float(sum(weights))
    w = [f32(n / total) for n in weights]
    x0 = x0.double().numpy()
    D = np.zeros_like(x0)
    A = np.zeros_like(x0)
    for wi, ci, th in zip(w, clip, thetas):
        d = th.double().numpy() - x0
        D += wi * ci * d
        A += np.abs(wi * ci * d)
    W = sum(w)
    delta, A = D / W, A / W
    dD = (5 + 2 * len(w)) * E * A
    ad = np.abs(delta)
    lr, b1, b2, tau = opt.lr, opt.beta1, opt.beta2, opt.tau
    if not is_param:
        x = x0 + delta
        return {"x": (x, K2 * (dD + E * np.abs(x)))}
    m0 = m0.double().numpy()
    if opt.name == "fedavgm":
        m = b1 * m0 + delta
        dm = dD + E * np.abs(m)
        x = x0 + lr * m
        return {"x": (x, K2 * (lr * dm + E * np.abs(x))), "m": (m, K2 * dm)}
    v0 = v0.double().numpy()
    m = b1 * m0 + (1 - b1) * delta
    dm = (1 - b1) * (dD + 2 * E * ad) + E * np.abs(m)
    d2 = delta * delta
    if opt.name == "fedadagrad":
        v = v0 + d2
        dv = 2 * ad * dD + E * v
    elif opt.name == "fedadam":
        v = b2 * v0 + (1 - b2) * d2
        dv = (1 - b2) * (2 * ad * dD + 3 * E * d2) + E * v
    else:
        v = v0 - (1 - b2) * d2 * np.sign(v0 - d2)
        dv = (1 - b2) * (2 * ad * dD + 3 * E * d2) + E * np.abs(v)
        near = np.abs(v0 - d2) <= 2 * ad * dD + 2 * E * d2
        dv = dv + np.where(near, 2 * (1 - b2) * d2, 0.0)
    denom = np.sqrt(v) + tau
    rd = dv / (2 * v) + 2 * E
    dq = (dm + np.abs(m) * (rd + E)) / denom
    x = x0 + lr * m / denom
    return {"x": (x, K2 * (lr * dq + E * np.abs(x))), "m": (m, K2 * dm),
            "v": (v, K2 * dv)}


def ratio(got, ref, bound):
    diff = np.abs(got.double().numpy() - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


@pytest.mark.parametrize("name", MODES)
@pytest.mark.parametrize("clip", [0.0, 0.2], ids=["noclip", "clip"])
def test_modes_against_float64(name, clip):
    model = make_model(0)
    global_sd = model.state_dict()
    pnames = param_names(model)
    weights = [96, 288, 160]
    opt = ServerOptimizer(name, client_clip_norm=clip, **HP)
    worst = 0.0
    for rnd in range(3):
        clients = clients_for(sd_of(model), rnd)
        if rnd == 0:
            opt._ensure_state(global_sd, pnames)
            tau2 = f32(f32(HP["tau"]) * f32(HP["tau"]))
            assert all((m == 0).all() for m in opt.m.values())
            assert all((v == tau2).all() for v in opt.v.values())
            assert set(opt.m) == set(pnames)
            assert set(opt.v) == (set(pnames) if name != "fedavgm" else set())
        x0 = {k: t.clone() for k, t in opt.x.items()}
        m0 = {k: t.clone() for k, t in opt.m.items()}
        v0 = {k: t.clone() for k, t in opt.v.items()}
        opt.step_(global_sd, clients, weights, pnames)
        assert opt.applied and opt.finite == [True] * 3
        # the clients' norms and coefficients, float64 from the stored inputs
        coefs = []
        for i, sd in enumerate(clients):
            nrm = math.sqrt(sum(
                float((sd[k].double() - x0[k].double()).pow(2).sum())
                for k in x0))
            c = min(1.0, (clip or math.inf) / (nrm + 1e-6))
            assert abs(opt.norm[i] / nrm - 1.0) <= 2 * E
            assert abs(opt.coef[i] / c - 1.0) <= 4 * E
            coefs.append(c)
        if clip == 0.0:
            assert opt.coef == [1.0] * 3                # exactly 1.0f
        else:
            assert max(coefs) < 1.0                     # every client clipped
        for k in x0:
            ref = round_ref(opt, k, k in pnames, x0[k], m0.get(k), v0.get(k),
                            [sd[k] for sd in clients], weights, coefs)
            got = {"x": opt.x[k], "m": opt.m.get(k), "v": opt.v.get(k)}
            for s in ref:
                worst = max(worst, ratio(got[s], *ref[s]))
            # the model receives the master in its own dtype
            assert bits_equal(global_sd[k], opt.x[k].to(global_sd[k].dtype))
        # integer buffers: the heaviest client's
        assert torch.equal(global_sd["1.num_batches_tracked"],
                           clients[1]["1.num_batches_tracked"])
    print(f"{name} clip={clip}: worst {worst:.3f} of the bound")
    assert worst <= 1.0
    assert opt.skipped_rounds == 0


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


def test_none_is_fedavg_bit_for_bit():
    assert ServerOptConfig().name == "none" and not ServerOptConfig().enabled
    model, twin = make_model(0), make_model(0)
    exp = Experiment(model, "plain", app=None)
    assert exp.server_opt is None
    assert "skipped_rounds" not in exp.metrics
    weights = [96, 288, 160]
    for rnd in range(2):
        clients = clients_for(sd_of(twin), rnd)
        _run_round(exp, _responses(clients, weights))
        fedavg_(twin.state_dict(), clients, weights)
        for k, t in model.state_dict().items():
            assert bits_equal(t, twin.state_dict()[k]), k


def test_fedavgm_with_unit_step_is_the_mean_of_clipped_updates():
    """b1 = 0, lr = 1, no clipping: x + sum w_i (theta_i - x) / W, which is
    FedAvg up to the rounding of the update form."""
    model, twin = make_model(0), make_model(0)
    opt = ServerOptimizer("fedavgm", lr=1.0, beta1=0.0)
    clients = clients_for(sd_of(model), 0)
    weights = [96, 288, 160]
    opt.step_(model.state_dict(), clients, weights, param_names(model))
    fedavg_(twin.state_dict(), clients, weights)
    for k, t in model.state_dict().items():
        if t.is_floating_point():
            assert torch.allclose(t, twin.state_dict()[k], rtol=0, atol=1e-6)
        else:
            assert torch.equal(t, twin.state_dict()[k])


@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_a_non_finite_client_is_left_out(bad):
    """Weights 1, 1, 2 with the last client poisoned: w = 1/4, 1/4 and W = 1/2,
    against the run of the two good clients alone, w = 1/2, 1/2 and W = 1.
    All of these are powers of two, so both runs round the same numbers and
    the results agree bit for bit."""
    for name in MODES:
        a, b = make_model(0), make_model(0)
        clients = clients_for(sd_of(a), 0)
        key = "0.weight"
        clients[2][key] = clients[2][key].clone()
        clients[2][key][3, 2] = bad
        oa = ServerOptimizer(name, client_clip_norm=0.2, **HP)
        ob = ServerOptimizer(name, client_clip_norm=0.2, **HP)
        oa.step_(a.state_dict(), clients, [1, 1, 2], param_names(a))
        ob.step_(b.state_dict(), clients[:2], [1, 1], param_names(b))
        assert oa.finite == [True, True, False] and oa.coef[2] == 0.0
        assert oa.last_W == 0.5 and ob.last_W == 1.0
        assert oa.skipped_rounds == 0
        for k, t in a.state_dict().items():
            if t.is_floating_point():
                assert torch.isfinite(t).all()
                assert bits_equal(t, b.state_dict()[k]), (name, k)
        for sa, sb in ((oa.x, ob.x), (oa.m, ob.m), (oa.v, ob.v)):
            assert all(bits_equal(sa[k], sb[k]) for k in sa)
        # the integer buffers still follow the heaviest client
        assert torch.equal(a.state_dict()["1.num_batches_tracked"],
                           clients[2]["1.num_batches_tracked"])


def test_all_clients_non_finite_skips_the_round():
    for name in MODES:
        model = make_model(0)
        pn = param_names(model)
        opt = ServerOptimizer(name, **HP)
        opt.step_(model.state_dict(), clients_for(sd_of(model), 0),
                  [96, 288, 160], pn)                   # state becomes non-zero
        before = {k: t.clone() for k, t in opt.state_dict().items()}
        model_before = sd_of(model)
        clients = clients_for(sd_of(model), 1)
        for sd in clients:
            sd["0.bias"][0] = math.nan
        opt.step_(model.state_dict(), clients, [96, 288, 160], pn)
        assert not opt.applied and opt.skipped_rounds == 1
        assert opt.last_W == 0.0 and opt.finite == [False] * 3
        after = opt.state_dict()
        assert int(after.pop("skipped_rounds")) == 1
        before.pop("skipped_rounds")
        assert all(bits_equal(after[k], before[k]) for k in before)
        for k, t in model.state_dict().items():
            if t.is_floating_point():                   # reset to the global x
                assert bits_equal(t, model_before[k])
        opt.step_(model.state_dict(), clients_for(sd_of(model), 2),
                  [96, 288, 160], pn)                   # the next round trains
        assert opt.applied and opt.skipped_rounds == 1
        assert not bits_equal(model.state_dict()["0.weight"],
                              model_before["0.weight"])


@pytest.mark.parametrize("max_norm", [0.05, 0.3, 100.0])
def test_clip_coefficient_is_torchs_rule(max_norm):
    model = make_model(0)
    clients = clients_for(sd_of(model), 0)
    opt = ServerOptimizer("fedavgm", client_clip_norm=max_norm)
    g0 = sd_of(model)
    opt.step_(model.state_dict(), clients, [1, 1, 1], param_names(model))
    for i, sd in enumerate(clients):
        grads = []
        for k, t in g0.items():
            if t.is_floating_point():
                p = nn.Parameter(torch.zeros_like(t))
                p.grad = sd[k] - t
                grads.append(p)
        before = [p.grad.clone() for p in grads]
        total = torch.nn.utils.clip_grad_norm_(grads, max_norm)
        assert float(total) == pytest.approx(opt.norm[i], rel=1e-6)
        j = max(range(len(before)), key=lambda j: before[j].abs().max())
        idx = before[j].abs().argmax()
        torch_coef = float(grads[j].grad.reshape(-1)[idx]
                           / before[j].reshape(-1)[idx])
        assert opt.coef[i] == pytest.approx(torch_coef, rel=1e-6)
        assert (opt.coef[i] == 1.0) == (float(total) + 1e-6 <= max_norm)


def test_yogi_sign():
    """v above, below and equal to d2, on one tensor."""
    tau = 0.5
    opt = ServerOptimizer("fedyogi", lr=0.1, beta1=0.0, beta2=0.75, tau=tau)
    g = OrderedDict(w=torch.zeros(3))
    # v0 = tau^2 = 0.25; Delta = 0.25, 0.5, 2: d2 = 0.0625, 0.25, 4
    client = OrderedDict(w=torch.tensor([0.25, 0.5, 2.0]))
    opt.step_(g, [client], [1], ["w"])
    assert opt.last_W == 1.0
    # v = v0 - 0.25 d2 sign(v0 - d2)
    assert opt.v["w"].tolist() == [0.25 - 0.25 * 0.0625, 0.25, 0.25 + 1.0]
    m = opt.m["w"]
    assert m.tolist() == [0.25, 0.5, 2.0]
    want = 0.1 * m.double() / (opt.v["w"].double().sqrt() + tau)
    assert torch.allclose(opt.x["w"].double(), want, rtol=4 * E, atol=0)


def test_fp32_master_keeps_what_bf16_loses():
    ulp = 2.0 ** -7
    opt = ServerOptimizer("fedavgm", lr=0.4, beta1=0.0)
    g = OrderedDict(w=torch.ones(4, dtype=torch.bfloat16))
    seen = []
    for _ in range(2):
        client = OrderedDict(w=torch.full((4,), 1.0 + ulp,
                                          dtype=torch.bfloat16))
        opt.step_(g, [client], [5], ["w"])
        seen.append((opt.x["w"].clone(), g["w"].float().clone()))
    (x1, t1), (x2, t2) = seen
    assert (x1 > 1.0).all() and (x1 < 1.0 + 0.5 * ulp).all()
    assert (t1 == 1.0).all()
    assert (x2 > 1.0 + 0.5 * ulp).all() and (t2 == 1.0 + ulp).all()


def test_sidecar_checkpoint_round_trip(tmp_path):
    cfg = BatonConfig(checkpoint_dir=str(tmp_path))
    cfg.server_opt = ServerOptConfig(name="fedadam", client_clip_norm=0.2,
                                     **HP)
    weights = [96, 288, 160]
    exp = Experiment(make_model(0), "exp", app=None, config=cfg)
    assert exp.metrics["skipped_rounds"] == 0
    for rnd in range(2):
        _run_round(exp, _responses(clients_for(sd_of(exp.model), rnd),
                                   weights))
    poisoned = clients_for(sd_of(exp.model), 2)
    for sd in poisoned:
        sd["0.weight"][0, 0] = math.inf
    _run_round(exp, _responses(poisoned, weights))
    assert exp.metrics["skipped_rounds"] == 1
    assert exp.metrics["last_round_W"] == 0.0
    assert (tmp_path / "exp.server_opt.ckpt").exists()
    # the checkpoint itself is what it was: the round-start payload
    from baton_amd.control.wire import decode_payload

    meta, tensors = decode_payload((tmp_path / "exp.ckpt").read_bytes())
    assert list(tensors) == list(exp.model.state_dict())
    assert set(meta) == {"update_name", "n_epoch", "round_index",
                         "loss_history"}

    again = Experiment(make_model(7), "exp", app=None, config=cfg)
    assert again.load_checkpoint()
    assert again.server_opt.skipped_rounds == 1
    assert again.metrics["skipped_rounds"] == 1
    a, b = exp.server_opt.state_dict(), again.server_opt.state_dict()
    assert list(a) == list(b)
    assert all(bits_equal(a[k], b[k]) for k in a)
    # both continue identically
    clients = clients_for(sd_of(exp.model), 3)
    _run_round(exp, _responses(clients, weights))
    _run_round(again, _responses(clients, weights))
    for k, t in exp.model.state_dict().items():
        assert bits_equal(t, again.model.state_dict()[k]), k
    assert exp.metrics["last_round_W"] == again.metrics["last_round_W"] > 0.99

    # another optimizer's sidecar is refused, a missing one is not an error
    cfg2 = BatonConfig(checkpoint_dir=str(tmp_path))
    cfg2.server_opt = ServerOptConfig(name="fedyogi")
    with pytest.raises(ValueError, match="fedadam"):
        Experiment(make_model(0), "exp", app=None, config=cfg2).load_checkpoint()
    plain = Experiment(make_model(0), "exp", app=None,
                       config=BatonConfig(checkpoint_dir=str(tmp_path)))
    assert plain.load_checkpoint() and plain.server_opt is None


def test_config_round_trip_and_refusals(tmp_path):
    raw = {"server_opt": {"name": "fedyogi", "lr": 0.03, "beta1": 0.8,
                          "beta2": 0.9, "tau": 0.01, "client_clip_norm": 2.0}}
    cfg = BatonConfig.from_dict(raw)
    assert cfg.server_opt == ServerOptConfig("fedyogi", 0.03, 0.8, 0.9, 0.01,
                                             2.0)
    assert cfg.server_opt.enabled
    again = BatonConfig.from_dict(
        {k: v for k, v in cfg.to_dict().items() if v is not None})
    assert again.server_opt == cfg.server_opt
    path = tmp_path / "baton.toml"
    path.write_text('[server_opt]\nname = "fedadam"\nlr = 0.5\n'
                    "client_clip_norm = 1.5\n")
    toml = BatonConfig.from_toml(str(path))
    assert toml.server_opt == ServerOptConfig(name="fedadam", lr=0.5,
                                              client_clip_norm=1.5)
    default = BatonConfig()
    assert default.server_opt == ServerOptConfig("none", 1.0, 0.9, 0.99, 1e-3,
                                                 0.0)
    assert ServerOptimizer.from_config(default.server_opt) is None
    opt = ServerOptimizer.from_config(cfg.server_opt)
    assert (opt.name, opt.lr, opt.client_clip_norm) == ("fedyogi", f32(0.03),
                                                        2.0)
    assert ServerOptimizer("fedavgm").client_clip_norm == math.inf

    with pytest.raises(KeyError, match="ServerOptConfig.momentum"):
        BatonConfig.from_dict({"server_opt": {"momentum": 0.9}})
    bad = [dict(name="fedlion"), dict(lr=0.0), dict(lr=-1.0),
           dict(lr=math.nan), dict(beta1=1.0), dict(beta1=-0.1),
           dict(beta2=1.0), dict(beta2=math.nan), dict(tau=0.0),
           dict(tau=math.nan), dict(client_clip_norm=-1.0),
           dict(client_clip_norm=math.nan)]
    for kw in bad:
        kw = {"name": "fedadam", **kw}
        with pytest.raises(ValueError):
            ServerOptConfig(**kw)
        with pytest.raises(ValueError):
            BatonConfig.from_dict({"server_opt": kw})
        with pytest.raises(ValueError):
            ServerOptimizer(**kw)
    ServerOptConfig(name="fedavgm", tau=0.0)           # tau is the adaptive modes'
    with pytest.raises(ValueError):
        ServerOptConfig(name="none", lr=-1.0)          # checked even when off
    with pytest.raises(ValueError):
        ServerOptimizer("none")

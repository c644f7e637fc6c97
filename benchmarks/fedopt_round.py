"""One federated round on the data plane at world 1 (RCCL): plain
``fedavg_arena`` against ``fedopt_arena`` with a server optimizer.

    python benchmarks/fedopt_round.py [--rounds 9] [--iters 10] [--out FILE]

Per arena size (one bf16 parameter group; random data generated on the
device) it times, between device events on the compute stream, ``iters``
synchronous rounds of

    fedavg    ``fedavg_arena`` (the code every earlier benchmark ran)
    fedavg2   the same call again: its distance from ``fedavg`` is the
              run-to-run spread the other figures are read against
    fedavgm   ``fedopt_arena`` with server momentum
    fedadam   ``fedopt_arena`` with the adaptive step

all on the same arena, each variant with its own data plane object (side
stream, reduce buffer, server state) on the one process group. Sizes: the
ResNet-18 arena (11.7 M elements) and the BERT-base arena (110 M).

The variants run interleaved: each round times every variant in turn, and
the table gives the median, minimum and (max - min) / median over the rounds,
the ratio to ``fedavg`` and, beside it, the ratio of bytes moved per element
as read from the kernels (bf16 theta, fp32 everything else):

    fedavg    scale_cast 2 + 4, cast_copy 4 + 2                     = 12 B
    fedopt    delta_sumsq 2 + 4, delta_scale_cast 2 + 4 + 4,
              server_step D 4 + x 8 (+ m 8) (+ v 8), cast_copy 4 + 2
                                              fedavgm 42 B, fedadam 50 B

At world 1 the reduce and the broadcast are self-copies inside RCCL; they are
issued and waited on as at any world size. A GPU is required."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("resnet18", 11_689_512), ("bert-base", 109_482_240)]
VARIANTS = ("fedavg", "fedavg2", "fedavgm", "fedadam")
BYTES = {"fedavg": 12, "fedavg2": 12, "fedavgm": 42, "fedadam": 50}


class _Flat(torch.nn.Module):
    """One parameter of n elements: the arena of a model of that size."""

    def __init__(self, n, dtype, device):
        super().__init__()
        self.w = torch.nn.Parameter(torch.empty(n, dtype=dtype, device=device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--arenas", default=",".join(s for s, _ in SIZES),
                    help="comma-separated subset of the arena sizes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fedopt_round.py measures on the GPU; none is visible")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29917")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    from baton_amd.parallel.data_plane import FederatedDataPlane
    from baton_amd.runtime.arena import FlatParamArena
    from baton_amd.utils.config import DataPlaneConfig, ServerOptConfig

    dev = torch.device("cuda", 0)
    results = []
    for label, n in SIZES:
        if label not in args.arenas.split(","):
            continue
        model = _Flat(n, torch.bfloat16, dev)
        gen = torch.Generator(device=dev).manual_seed(n)
        with torch.no_grad():
            model.w.copy_(torch.randn(n, generator=gen, device=dev).mul(0.02))
        arena = FlatParamArena(model, grads=False)
        planes = {}
        for name in VARIANTS:
            planes[name] = FederatedDataPlane(DataPlaneConfig(backend="nccl"),
                                              device=dev)
            if name in ("fedavgm", "fedadam"):
                planes[name].enable_server_opt(arena, ServerOptConfig(
                    name=name, lr=0.1, client_clip_norm=1.0))
        noise = torch.randn(n, generator=gen, device=dev).mul(1e-3).to(
            torch.bfloat16)
        flat = arena.groups[0].flat

        def one(name):
            flat.add_(noise)            # the client's local training, 6 B
            if planes[name].server_opt_enabled:
                planes[name].fedopt_arena(arena, 128)
            else:
                planes[name].fedavg_arena(arena, 128)

        def timed(name, call=True):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                one(name) if call else flat.add_(noise)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.iters * 1e3   # us

        for name in VARIANTS:
            for _ in range(args.warmup):
                one(name)
        torch.cuda.synchronize()
        times = {name: [] for name in VARIANTS}
        train = []
        for _ in range(args.rounds):
            for name in VARIANTS:
                times[name].append(timed(name))
            train.append(timed("fedavg", call=False))
        fill = statistics.median(train)
        base = statistics.median(times["fedavg"]) - fill
        for name, ts in times.items():
            med = statistics.median(ts)
            state = None
            if planes[name].server_opt_enabled:
                state = dict(clip_state=planes[name].fedopt_clip_state.tolist(),
                             round_state=planes[name].fedopt_round_state.tolist())
            results.append(dict(
                arena=label, n=n, variant=name, median_us=round(med - fill, 2),
                min_us=round(min(ts) - fill, 2),
                spread=round((max(ts) - min(ts)) / med, 4),
                vs_fedavg=round((med - fill) / base, 3),
                bytes_vs_fedavg=round(BYTES[name] / BYTES["fedavg"], 3),
                train_us=round(fill, 2), rounds=args.rounds, iters=args.iters,
                **(state or {})))
            print(json.dumps(results[-1]), flush=True)
        del planes, model, arena, noise, flat
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

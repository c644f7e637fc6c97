"""The server step with and without DP noise (ops/csrc/fedopt.hip), and the
noise generator alone.

    python benchmarks/dp_noise_step.py [--rounds 9] [--iters 20] [--out FILE]

Per arena size (ResNet-18, 11.7 M elements; BERT-base, 110 M) and per mode it
times, between device events, ``iters`` calls on one whole fp32 buffer of

    plain     ``ops.server_step`` (NOISE = false: the kernel as it always was)
    plain2    the same call again: its distance from ``plain`` is the
              run-to-run spread the other figures are read against
    noise     ``ops.server_step_noise`` (Philox4x32-10 + Box-Muller in the pass)

and, once per size, ``ops.dp_noise`` alone (4 B written per element). The
variants run interleaved: each round times every variant in turn, and the
table gives the median, minimum and (max - min) / median over the rounds, the
achieved bytes per second from the bytes the kernel moves per element

    mean 12 B (D 4, x 8), fedavgm 20 B (+ m 8), adaptive 28 B (+ v 8)

and, for ``noise``, the ratio to ``plain``. On an extension without the noise
entries (an earlier commit) only ``plain`` and ``plain2`` are timed, so the
same script gives the line to compare against. A GPU is required."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("resnet18", 11_689_512), ("bert-base", 109_482_240)]
MODES = ("mean", "fedavgm", "fedadagrad", "fedadam", "fedyogi")
BYTES = {"mean": 12, "fedavgm": 20, "fedadagrad": 28, "fedadam": 28,
         "fedyogi": 28, "dp_noise": 4}
HP = (0.1, 0.9, 0.99, 1e-3)
SEED, SIGMA = 0x5EED5EED5EED5EED, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--arenas", default=",".join(s for s, _ in SIZES),
                    help="comma-separated subset of the arena sizes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dp_noise_step.py measures on the GPU; none is visible")
    from baton_amd.ops._ext import require_hip

    ops = require_hip()
    has_noise = hasattr(ops, "server_step_noise")
    dev = torch.device("cuda", 0)
    results = []
    for label, n in SIZES:
        if label not in args.arenas.split(","):
            continue
        gen = torch.Generator(device=dev).manual_seed(n)
        D = torch.randn(n, generator=gen, device=dev).mul(1e-3)
        x = torch.randn(n, generator=gen, device=dev).mul(0.02)
        m = torch.zeros(n, device=dev)
        v = torch.full((n,), 1e-6, device=dev)
        rs = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)
        out = torch.empty(n, device=dev)
        rnd = [0]

        def call(mode, variant):
            a = (mode, D, x, None if mode == "mean" else m,
                 v if mode in MODES[2:] else None, *HP, rs)
            if variant == "noise":
                rnd[0] += 1
                ops.server_step_noise(*a, SEED, rnd[0], 0, 0, SIGMA)
            elif variant == "dp_noise":
                rnd[0] += 1
                ops.dp_noise(out, SEED, rnd[0], 0, 0, SIGMA)
            else:
                ops.server_step(*a)

        def timed(mode, variant):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                call(mode, variant)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.iters * 1e3   # us

        cases = [(mode, var) for mode in MODES
                 for var in (("plain", "plain2", "noise") if has_noise
                             else ("plain", "plain2"))]
        if has_noise:
            cases.append(("dp_noise", "dp_noise"))
        for case in cases:
            for _ in range(args.warmup):
                call(*case)
        torch.cuda.synchronize()
        times = {case: [] for case in cases}
        for _ in range(args.rounds):
            for case in cases:
                times[case].append(timed(*case))
        for (mode, var), ts in times.items():
            med = statistics.median(ts)
            row = dict(arena=label, n=n, mode=mode, variant=var,
                       median_us=round(med, 2), min_us=round(min(ts), 2),
                       spread=round((max(ts) - min(ts)) / med, 4),
                       gb_per_s=round(BYTES[mode] * n / med / 1e3, 1),
                       rounds=args.rounds, iters=args.iters)
            if var != "dp_noise":
                row["vs_plain"] = round(
                    med / statistics.median(times[(mode, "plain")]), 4)
            results.append(row)
            print(json.dumps(row), flush=True)
        assert bool(torch.isfinite(x).all()), "x left the finite range"
        del D, x, m, v, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

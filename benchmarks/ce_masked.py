"""Fused cross-entropy forward + backward with ignored labels, against the
dense call, at the two vocabulary-head shapes of the transformer models.

    python benchmarks/ce_masked.py [--rounds 9] [--iters 20] [--out FILE]

Per shape (bf16 logits [rows, C], random data generated on the device) it
times forward + backward of the raw ops for

    dense      ``ce_fwd`` + ``ce_bwd`` (the dense kernels, unchanged code)
    dense2     the same call again: its distance from ``dense`` is the
               run-to-run spread the other figures are read against
    all_live   ``ce_masked_fwd`` + ``ce_masked_bwd``, ignore_index = -100 and
               no such label: the cost of the feature when nothing is ignored
    half       the same with every second row's label -100. The grid is 2048
               blocks striding over the rows, an even stride: every block
               sees only live or only ignored rows, so half the blocks do all
               the row reads
    half_rand  a random half of the rows ignored (seeded): live and ignored
               rows mix inside every block's walk, but unevenly (a block has
               2 to 5 rows here), and the kernel lasts as long as its
               longest block
    half_trip  rows r with (r / 2048) odd ignored: every block's walk
               alternates live and ignored rows, the balanced case (what an
               even spread of the live rows over the blocks would give);
               ``live`` in the output is the share of live rows

Shapes: the BERT head (9830 masked rows of a 512 x 128 batch at 15 %,
C = 30528) and a Llama head (4088 = 8 x 511 next-token rows, C = 128256).

The variants run interleaved in one process: each round times ``iters``
forward + backward pairs of every variant in turn between device events, and
the table gives the median, minimum and (max - min) / median over the rounds.
``fwd_median_us`` is the forward alone, timed the same way in the same rounds.
Before timing, the all_live lse and dx are compared bit for bit with the dense
ones at the timed size. A GPU is required; there is no CPU path."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(9830, 30528), (4088, 128256)]
VARIANTS = ("dense", "dense2", "all_live", "half", "half_rand", "half_trip")
KMAXGRID = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ce_masked.py measures on the GPU; none is visible")
    from baton_amd.ops._ext import require_hip

    ops = require_hip()
    dev = "cuda:0"
    results = []
    for R, C in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(R)
        x = torch.randn(R, C, generator=gen, device=dev).mul(3.0).to(
            torch.bfloat16)
        t = torch.randint(0, C, (R,), generator=gen, device=dev)
        t_half = t.clone()
        t_half[1::2] = -100
        t_rand = t.clone()
        t_rand[torch.randperm(R, generator=gen, device=dev)[:R // 2]] = -100
        t_trip = t.clone()
        t_trip[(torch.arange(R, device=dev) // KMAXGRID) % 2 == 1] = -100
        targets = {"all_live": t, "half": t_half, "half_rand": t_rand,
                   "half_trip": t_trip}
        dout = torch.ones((), device=dev)

        def step(name, bwd=True):
            if name in ("dense", "dense2"):
                _, lse = ops.ce_fwd(x, t)
                return lse, ops.ce_bwd(x, t, lse, dout) if bwd else None
            tt = targets[name]
            _, lse, nv = ops.ce_masked_fwd(x, tt, -100)
            return lse, (ops.ce_masked_bwd(x, tt, lse, nv, dout, -100)
                         if bwd else None)

        def timed(name, bwd):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                step(name, bwd)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.iters * 1e3   # us

        lse_d, dx_d = step("dense")
        lse_m, dx_m = step("all_live")
        same = bool(torch.equal(lse_d.view(torch.int32), lse_m.view(torch.int32))
                    and torch.equal(dx_d.view(torch.int16),
                                    dx_m.view(torch.int16)))
        del lse_d, dx_d, lse_m, dx_m
        for n in VARIANTS:
            for _ in range(args.warmup):
                step(n)
        torch.cuda.synchronize()
        times = {n: [] for n in VARIANTS}
        fwd = {n: [] for n in VARIANTS}
        for _ in range(args.rounds):
            for n in VARIANTS:
                times[n].append(timed(n, True))
                fwd[n].append(timed(n, False))
        base = statistics.median(times["dense"])
        for n, ts in times.items():
            med = statistics.median(ts)
            results.append(dict(
                rows=R, C=C, variant=n, median_us=round(med, 2),
                min_us=round(min(ts), 2),
                spread=round((max(ts) - min(ts)) / med, 4),
                vs_dense=round(med / base, 4),
                live=round(float((targets[n] >= 0).float().mean()), 4)
                if n in targets else 1.0,
                fwd_median_us=round(statistics.median(fwd[n]), 2),
                all_live_bits_equal_dense=same,
                rounds=args.rounds, iters=args.iters))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""The fused Adam step with global-norm clipping, the non-finite skip and
decoupled decay, against the dense step, at two buffer sizes.

    python benchmarks/optim_clip.py [--rounds 9] [--iters 20] [--out FILE]

Per size (one flat buffer, random data generated on the device, gradients of
unit variance) it times ``FusedAdam.step()`` over a one-group arena stand-in,
all variants stepping the same parameter, gradient and moment buffers, for

    dense    ``adam_step`` (the dense kernel, unchanged code)
    dense2   the same optimizer again: its distance from ``dense`` is the
             run-to-run spread the other figures are read against
    inf      ``max_grad_norm=inf``: grad_sumsq + clip_finalize + the EXT step
             with coef == 1, the cost of measuring the norm and of the skip
             guard
    clipped  ``max_grad_norm=1.0``, far below the norm: the same launches
             with coef < 1
    adamw    ``decoupled_weight_decay=True`` without clipping: the EXT step
             alone (clip_state null)

Sizes: the BERT-base arena (110 M bf16 elements) and an fp32 group of 25 M
elements. The step zeroes the gradient as the arena step does, so every
variant also refills it; the refill (one device copy, the same for all) is
timed alone as ``refill_us`` and is part of every figure.

The variants run interleaved in one process: each round times ``iters`` steps
of every variant in turn between device events, and the table gives the
median, minimum and (max - min) / median over the rounds. A GPU is required;
there is no CPU path."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(110_000_000, torch.bfloat16), (25_000_000, torch.float32)]
VARIANTS = ("dense", "dense2", "inf", "clipped", "adamw")


class _Group:
    def __init__(self, flat, grad):
        self.flat, self.grad = flat, grad


class _Arena:
    """One dtype group, the shape ``from_arena`` reads."""

    def __init__(self, flat, grad):
        self.groups = [_Group(flat, grad)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_clip.py measures on the GPU; none is visible")
    from baton_amd.ops.optim import FusedAdam

    dev = "cuda:0"
    results = []
    for n, dtype in SIZES:
        gen = torch.Generator(device=dev).manual_seed(n)
        src = torch.randn(n, generator=gen, device=dev).to(dtype)
        kw = dict(lr=1e-4, weight_decay=0.01)
        extra = {"dense": {}, "dense2": {},
                 "inf": dict(max_grad_norm=float("inf")),
                 "clipped": dict(max_grad_norm=1.0),
                 "adamw": dict(decoupled_weight_decay=True)}
        # every variant steps the SAME p, g, m, v: which allocation a buffer
        # got moves the step time by more than the feature does
        # (profiles/r09_grad_clip.md)
        flat = torch.randn(n, generator=gen, device=dev).mul(0.02).to(dtype)
        arena = _Arena(flat, torch.zeros_like(flat))
        opts = {}
        for name in VARIANTS:
            opts[name] = FusedAdam.from_arena(arena, **kw, **extra[name])
            opts[name].exp_avg = opts["dense"].exp_avg
            opts[name].exp_avg_sq = opts["dense"].exp_avg_sq

        def step(name, do_step=True):
            o = opts[name]
            o._arena_grads[0].copy_(src)
            if do_step:
                o.step()

        def timed(name, do_step=True):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                step(name, do_step)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.iters * 1e3   # us

        for name in VARIANTS:
            for _ in range(args.warmup):
                step(name)
        torch.cuda.synchronize()
        state = {name: (o.clip_state.tolist() if o.clip_state is not None
                        else None) for name, o in opts.items()}
        times = {name: [] for name in VARIANTS}
        refill = []
        for _ in range(args.rounds):
            for name in VARIANTS:
                times[name].append(timed(name))
            refill.append(timed("dense", do_step=False))
        base = statistics.median(times["dense"])
        fill = statistics.median(refill)
        for name, ts in times.items():
            med = statistics.median(ts)
            results.append(dict(
                n=n, dtype=str(dtype).replace("torch.", ""), variant=name,
                median_us=round(med, 2), min_us=round(min(ts), 2),
                spread=round((max(ts) - min(ts)) / med, 4),
                vs_dense=round(med / base, 4),
                step_only_vs_dense=round((med - fill) / (base - fill), 4),
                refill_us=round(fill, 2), clip_state=state[name],
                skipped=opts[name].skipped_steps(),
                rounds=args.rounds, iters=args.iters))
            print(json.dumps(results[-1]), flush=True)
        del opts, src, flat, arena
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Flash attention forward + backward with per-sequence lengths, against the
dense call, at the BERT-base attention shape.

    python benchmarks/flash_varlen.py [--rounds 9] [--iters 20] [--out FILE]

Per shape ([B,S,3,h,dh] packed qkv as BertSelfAttention produces it, bf16,
random data) it times ``flash_fwd`` + ``flash_bwd`` for

    dense     the plain call (the dense kernels, unchanged code)
    dense2    the same call again: its distance from ``dense`` is the
              run-to-run spread the other figures are read against
    full      seq_lens given, every L_b = S: the cost of the feature when
              nothing is padded
    uniform   L_b uniform in [S/4, S]
    half      every L_b = S/2

The variants run interleaved in one process: each round times ``iters``
forward + backward pairs of every variant in turn between device events, and
the table gives the median, minimum and (max - min) / median over the rounds.
Score work of a variant is sum_b L_b^2 / (B S^2) of the dense call's.
A GPU is required; there is no CPU path."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # B, S, h, dh: the bench.py BERT-base step (batch 512, S = 128), and the
    # same number of tokens at S = 512
    (512, 128, 12, 64),
    (128, 512, 12, 64),
]


def variants(B, S, gen):
    full = torch.full((B,), S, dtype=torch.int32)
    uni = torch.randint(S // 4, S + 1, (B,), generator=gen, dtype=torch.int32)
    half = torch.full((B,), S // 2, dtype=torch.int32)
    return {"dense": None, "dense2": None, "full": full, "uniform": uni,
            "half": half}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("flash_varlen.py measures on the GPU; none is visible")
    from baton_amd.ops._ext import require_hip

    ops = require_hip()
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    results = []
    for B, S, h, dh in SHAPES:
        qkv = torch.randn(B, S, 3, h, dh, generator=gen).to(torch.bfloat16)
        dout = torch.randn(B, S, h, dh, generator=gen).to(torch.bfloat16)
        qkv, dout = qkv.to(dev), dout.to(dev)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        o = torch.empty(B, S, h, dh, dtype=torch.bfloat16, device=dev)
        dqkv = torch.empty_like(qkv)
        var = variants(B, S, gen)
        lens = {n: (None if t is None else t.to(dev)) for n, t in var.items()}

        def step(sl):
            extra = () if sl is None else (sl,)
            _, lse = ops.flash_fwd(q, k, v, o, False, *extra)
            ops.flash_bwd(q, k, v, o, dout, lse, dqkv[:, :, 0], dqkv[:, :, 1],
                          dqkv[:, :, 2], False, *extra)

        for n in var:
            for _ in range(args.warmup):
                step(lens[n])
        torch.cuda.synchronize()
        times = {n: [] for n in var}
        for _ in range(args.rounds):
            for n in var:
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    step(lens[n])
                t1.record()
                t1.synchronize()
                times[n].append(t0.elapsed_time(t1) / args.iters * 1e3)  # us
        base = statistics.median(times["dense"])
        for n, ts in times.items():
            med = statistics.median(ts)
            work = 1.0 if var[n] is None else \
                float((var[n].double() ** 2).sum() / (B * S * S))
            results.append(dict(
                B=B, S=S, h=h, dh=dh, variant=n, median_us=round(med, 2),
                min_us=round(min(ts), 2),
                spread=round((max(ts) - min(ts)) / med, 4),
                vs_dense=round(med / base, 4), score_work=round(work, 4),
                rounds=args.rounds, iters=args.iters))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""The robust aggregation kernel (ops/csrc/fedrobust.hip) beside the server
step in ``mean`` mode.

    python benchmarks/robust_agg.py [--rounds 9] [--iters 10] [--out FILE]

Per arena size (ResNet-18, 11.7 M elements; BERT-base, 109.5 M) it times,
between device events, ``iters`` calls on one whole fp32 buffer of

    mean      ``ops.server_step("mean", ...)``: 12 B per element (D 4, x 8),
              the yardstick of a bandwidth-bound pass on this device
    mean2     the same call again: its distance from ``mean`` is the
              run-to-run spread the other figures are read against
    median, trimmed_mean (beta = 0.2) at K in {4, 8, 16}
              ``ops.robust_select`` over K rows with all of them live:
              (K + 1) * 4 B per element (K rows read, D written)

The variants run interleaved: each round times every variant in turn, and the
table gives the median, minimum and (max - min) / median over the rounds and
the achieved bytes per second. A round of the data plane also gathers the K
rows over the links; that needs K devices and is not timed here.
``--arenas bucket`` times one bucket of the data plane's staging shape and
``--row-pad P`` puts P more elements between the rows of U, to see what the
distance between the rows costs. A GPU is required."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [("resnet18", 11_689_512), ("bert-base", 109_482_240)]
# one bucket of the data plane's staging buffer (rows 16 MiB apart); only
# with --arenas bucket
EXTRA_SIZES = [("bucket", 4 * 1024 * 1024)]
KS = (4, 8, 16)
AGGS = (("median", 0.0), ("trimmed_mean", 0.2))
HP = (0.1, 0.9, 0.99, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--arenas", default=",".join(s for s, _ in SIZES),
                    help="comma-separated subset of the arena sizes")
    ap.add_argument("--row-pad", type=int, default=0,
                    help="elements added to U's row stride (a multiple of 4)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("robust_agg.py measures on the GPU; none is visible")
    from baton_amd.fed.server_opt import trim_table
    from baton_amd.ops._ext import require_hip

    ops = require_hip()
    dev = torch.device("cuda", 0)
    results = []
    for label, n in SIZES + EXTRA_SIZES:
        if label not in args.arenas.split(","):
            continue
        gen = torch.Generator(device=dev).manual_seed(n)
        U = torch.randn(max(KS), n + args.row_pad, generator=gen,
                        device=dev).mul(1e-3)[:, :n]
        D = torch.empty(n, device=dev)
        Dm = torch.randn(n, generator=gen, device=dev).mul(1e-3)
        x = torch.randn(n, generator=gen, device=dev).mul(0.02)
        rs_mean = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)
        state = {}
        for K in KS:
            for agg, beta in AGGS:
                flags = torch.ones(K, device=dev)
                table = torch.tensor(trim_table(agg, beta, K),
                                     dtype=torch.int32, device=dev)
                rs = torch.zeros(4, device=dev)
                ag = torch.zeros(2, device=dev)
                ops.robust_finalize(flags, table, rs, ag)
                state[(agg, K)] = (flags, ag, rs)

        def call(variant, K):
            if K == 0:
                ops.server_step("mean", Dm, x, None, None, *HP, rs_mean)
            else:
                flags, ag, rs = state[(variant, K)]
                ops.robust_select(D, U[:K], flags, ag, rs)

        def timed(variant, K):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                call(variant, K)
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.iters * 1e3   # us

        cases = [("mean", 0), ("mean2", 0)] + [
            (agg, K) for K in KS for agg, _ in AGGS]
        for case in cases:
            for _ in range(args.warmup):
                call(*case)
        torch.cuda.synchronize()
        times = {case: [] for case in cases}
        for _ in range(args.rounds):
            for case in cases:
                times[case].append(timed(*case))
        mean_med = statistics.median(times[("mean", 0)])
        mean_tb = 12 * n / mean_med / 1e6
        for (variant, K), ts in times.items():
            med = statistics.median(ts)
            nbytes = 12 if K == 0 else (K + 1) * 4
            tb = nbytes * n / med / 1e6
            row = dict(arena=label, n=n, row_pad=args.row_pad,
                       variant=variant, K=K,
                       bytes_per_elem=nbytes, median_us=round(med, 2),
                       min_us=round(min(ts), 2),
                       spread=round((max(ts) - min(ts)) / med, 4),
                       tb_per_s=round(tb, 3),
                       vs_mean_tb=round(tb / mean_tb, 4),
                       rounds=args.rounds, iters=args.iters)
            results.append(row)
            print(json.dumps(row), flush=True)
        assert bool(torch.isfinite(D).all()), "D left the finite range"
        del U, D, Dm, x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

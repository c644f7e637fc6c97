"""robust_finalize and robust_select (ops/csrc/fedrobust.hip) on the GPU
against the oracle of fed/server_opt.py (``robust_counts``, ``robust_sum``,
``robust_delta``), by value with ``torch.equal``: the kernel sorts the same
numbers and adds them in the same order with one rounding per add, so there is
no tolerance. -0.0 and +0.0 may leave the sort in either order, which
``torch.equal`` does not tell apart.

U is a slice at element offset 8 of a NaN-filled parent with a row stride
larger than n; D sits inside a NaN parent whose other elements must keep
their bits. Planted per column c (after row K // 2 was scaled by 1e6):
c % 8 == 1 equal values across rows, c % 8 == 2 zeros of alternating sign,
c % 8 == 3 +3e38 in row 0 and -3e38 in row K - 1; random data makes the tail
differ from the last full vector."""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fedopt_exact import (  # noqa: E402
    DEV, PAD, bits, in_parent, native_ops, same_bits)

from baton_amd.fed.server_opt import (  # noqa: E402
    robust_counts, robust_delta, robust_sum, trim_table)

KS = [1, 2, 3, 5, 8, 16]
SIZES = [1, 3, 4, 5, 255 * 4 + 3, 256 * 4 + 1]
BIG = 4194333                       # past the capped grid: two passes and a tail
AGGS = [("median", 0.0), ("trimmed_mean", 0.0), ("trimmed_mean", 0.2),
        ("trimmed_mean", 0.49)]


def make_rows(K: int, n: int, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    U = torch.randn(K, n, generator=gen)
    U[K // 2] *= 1e6
    U[:, 1::8] = U[0, 1::8].clone()
    signs = torch.tensor([0.0, -0.0]).repeat(K)[:K].reshape(K, 1)
    U[:, 2::8] = signs
    U[0, 3::8] = 3e38
    U[K - 1, 3::8] = -3e38
    return U


def flag_patterns(K: int):
    """name -> flags: all live, one dead row, one live row, none."""
    pats = {"all": [1.0] * K, "none": [0.0] * K}
    if K >= 2:
        one_dead = [1.0] * K
        one_dead[K // 3] = 0.0
        pats["one_dead"] = one_dead
        k1 = [0.0] * K
        k1[K - 1] = 1.0
        pats["k1"] = k1
    return pats


def poison_dead_rows(U: torch.Tensor, flags) -> torch.Tensor:
    """A dead row holds NaN and 1e30: its content must never be used."""
    U = U.clone()
    for r, f in enumerate(flags):
        if f == 0.0:
            U[r, ::2] = math.nan
            U[r, 1::2] = 1e30
    return U


def strided_rows(U: torch.Tensor):
    """U at element offset PAD of the rows of a NaN parent whose row stride
    is larger than n and a multiple of 4: (parent, view)."""
    K, n = U.shape
    stride = (n + 3) // 4 * 4 + PAD + 4
    parent = torch.full((K, stride), math.nan, device=DEV)
    view = parent[:, PAD: PAD + n]
    view.copy_(U)
    assert view.stride() == (stride, 1) or K == 1 or n == 1
    return parent, view


def run_case(ops, U_dev, U_cpu, flags, table, skipped_before=5.0):
    """One finalize + select; returns nothing, asserts everything."""
    K, n = U_cpu.shape
    fl = torch.tensor(flags, device=DEV)
    bt = torch.tensor(table, dtype=torch.int32, device=DEV)
    rs = torch.tensor([9.0, 9.0, 9.0, skipped_before], device=DEV)
    ag = torch.full((2,), 9.0, device=DEV)
    parent, D = in_parent(torch.full((n,), math.nan))
    before = bits(parent).clone()
    ops.robust_finalize(fl, bt, rs, ag)
    ops.robust_select(D, U_dev, fl, ag, rs)
    torch.cuda.synchronize()
    k, b, kept, inv, applied = robust_counts(flags, table)
    assert ag.tolist() == [float(k), float(b)]
    assert rs.tolist() == [float(kept), inv, float(applied),
                           skipped_before + (0.0 if applied else 1.0)]
    # D's neighbours keep their bits
    after = bits(parent)
    assert torch.equal(after[:PAD], before[:PAD])
    assert torch.equal(after[PAD + n:], before[PAD + n:])
    if not applied:
        assert torch.equal(after, before)        # the sentinel stands
        return
    want = robust_sum(U_cpu, flags, table)
    got = D.cpu()
    assert torch.equal(got, want), (
        f"K={K} n={n} flags={flags} table={table}: "
        f"{int((got != want).sum())} elements differ")
    # Delta as the unchanged server step forms it: fl(D * round_state[1])
    assert torch.equal(got * rs[1].cpu(), robust_delta(U_cpu, flags, table))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_select_and_finalize_against_the_oracle(K):
    ops = native_ops()
    for n in SIZES:
        base = make_rows(K, n, seed=100 * K + n % 97)
        for name, flags in flag_patterns(K).items():
            U_cpu = poison_dead_rows(base, flags)
            _, U_dev = strided_rows(U_cpu)
            for agg, beta in AGGS:
                run_case(ops, U_dev, U_cpu, flags, trim_table(agg, beta, K))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 16])
def test_select_past_the_capped_grid(K):
    ops = native_ops()
    base = make_rows(K, BIG, seed=K)
    flags = flag_patterns(K)["one_dead"]
    U_cpu = poison_dead_rows(base, flags)
    _, U_dev = strided_rows(U_cpu)
    for agg, beta in (("median", 0.0), ("trimmed_mean", 0.2)):
        run_case(ops, U_dev, U_cpu, flags, trim_table(agg, beta, K))


@pytest.mark.gpu
def test_select_feeds_the_unchanged_server_step():
    """robust_select then server_step('mean'): x + Delta, value for value."""
    ops = native_ops()
    K, n = 5, 1031
    U_cpu = poison_dead_rows(make_rows(K, n, seed=7), [1, 1, 0, 1, 1])
    flags = [1.0, 1.0, 0.0, 1.0, 1.0]
    table = trim_table("median", 0.0, K)
    _, U_dev = strided_rows(U_cpu)
    fl = torch.tensor(flags, device=DEV)
    bt = torch.tensor(table, dtype=torch.int32, device=DEV)
    rs = torch.zeros(4, device=DEV)
    ag = torch.zeros(2, device=DEV)
    D = torch.empty(n, device=DEV)
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(8))
    x = x0.to(DEV)
    ops.robust_finalize(fl, bt, rs, ag)
    ops.robust_select(D, U_dev, fl, ag, rs)
    ops.server_step("mean", D, x, None, None, 1.0, 0.0, 0.0, 1e-3, rs)
    torch.cuda.synchronize()
    assert rs.tolist() == [2.0, 0.5, 1.0, 0.0] and ag.tolist() == [4.0, 1.0]
    assert torch.equal(x.cpu(), x0 + robust_delta(U_cpu, flags, table))
    # a round without a live row: nothing moves, the skip is counted
    fl.zero_()
    held = x.clone()
    D.fill_(math.nan)
    ops.robust_finalize(fl, bt, rs, ag)
    ops.robust_select(D, U_dev, fl, ag, rs)
    ops.server_step("mean", D, x, None, None, 1.0, 0.0, 0.0, 1e-3, rs)
    torch.cuda.synchronize()
    assert rs.tolist() == [0.0, 0.0, 0.0, 1.0] and ag.tolist() == [0.0, 0.0]
    assert same_bits(x, held) and torch.isnan(D).all()


@pytest.mark.gpu
def test_refusals_by_name():
    ops = native_ops()
    K, n = 4, 64
    f32 = dict(dtype=torch.float32, device=DEV)

    def args():
        return dict(D=torch.zeros(n, **f32), U=torch.zeros(K, n, **f32),
                    flags=torch.ones(K, **f32),
                    agg_state=torch.zeros(2, **f32),
                    round_state=torch.zeros(4, **f32),
                    b_table=torch.zeros(K + 1, dtype=torch.int32, device=DEV))

    def select(match, **kw):
        a = {**args(), **kw}
        with pytest.raises(RuntimeError, match=match):
            ops.robust_select(a["D"], a["U"], a["flags"], a["agg_state"],
                              a["round_state"])

    def finalize(match, **kw):
        a = {**args(), **kw}
        with pytest.raises(RuntimeError, match=match):
            ops.robust_finalize(a["flags"], a["b_table"], a["round_state"],
                                a["agg_state"])

    a = args()
    ops.robust_finalize(a["flags"], a["b_table"], a["round_state"],
                        a["agg_state"])
    ops.robust_select(a["D"], a["U"], a["flags"], a["agg_state"],
                      a["round_state"])
    select("robust_select: U must be fp32", U=torch.zeros(K, n, device=DEV,
                                                          dtype=torch.bfloat16))
    select("robust_select: D must be fp32",
           D=torch.zeros(n, device=DEV, dtype=torch.bfloat16))
    select("robust_select: U must be on the device", U=torch.zeros(K, n))
    select("robust_select: D must be on the GPU", D=torch.zeros(n))
    select("robust_select: flags must be on the GPU", flags=torch.ones(K))
    select("robust_select: U must be 2-D", U=torch.zeros(K * n, **f32))
    select("robust_select: U must have 1 to 16 rows, got 17",
           U=torch.zeros(17, n, **f32), flags=torch.ones(17, **f32))
    select("robust_select: U must have 1 to 16 rows, got 0",
           U=torch.zeros(0, n, **f32))
    select("robust_select: flags must have 4 elements, got 3",
           flags=torch.ones(3, **f32))
    select("robust_select: U's rows must have D's 64 elements, got 60",
           U=torch.zeros(K, 60, **f32))
    select("robust_select: U's row stride must be a multiple of 4",
           U=torch.zeros(K, n + 2, **f32)[:, :n])
    select("robust_select: U must be 16-byte aligned",
           U=torch.zeros(K, n + 4, **f32)[:, 1: n + 1])
    select("robust_select: D must be 16-byte aligned",
           D=torch.zeros(n + 4, **f32)[1: n + 1])
    select("robust_select: U must have unit inner stride",
           U=torch.zeros(K, 2 * n, **f32)[:, ::2])
    select("robust_select: agg_state must have 2 elements",
           agg_state=torch.zeros(4, **f32))
    select("robust_select: round_state must have 4 elements",
           round_state=torch.zeros(2, **f32))
    finalize("robust_finalize: flags must be fp32",
             flags=torch.ones(K, device=DEV, dtype=torch.int32))
    finalize("robust_finalize: flags must have 1 to 16 elements",
             flags=torch.ones(17, **f32),
             b_table=torch.zeros(18, dtype=torch.int32, device=DEV))
    finalize("robust_finalize: b_table must be int32",
             b_table=torch.zeros(K + 1, **f32))
    finalize("robust_finalize: b_table must have 5 elements",
             b_table=torch.zeros(K, dtype=torch.int32, device=DEV))
    finalize("robust_finalize: b_table must be on the device",
             b_table=torch.zeros(K + 1, dtype=torch.int32))
    finalize("robust_finalize: round_state must have 4 elements",
             round_state=torch.zeros(3, **f32))
    finalize("robust_finalize: agg_state must have 2 elements",
             agg_state=torch.zeros(3, **f32))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_finalize_clamps_a_bad_table():
    """kept >= 1 whatever the table holds: b is clamped to (k - 1) // 2."""
    ops = native_ops()
    fl = torch.tensor([1.0, 1.0, 0.0, 1.0], device=DEV)
    rs = torch.zeros(4, device=DEV)
    ag = torch.zeros(2, device=DEV)
    for entry, want_b in ((7, 1), (-3, 0)):
        bt = torch.full((5,), entry, dtype=torch.int32, device=DEV)
        ops.robust_finalize(fl, bt, rs, ag)
        assert ag.tolist() == [3.0, float(want_b)]
        kept = 3 - 2 * want_b
        assert rs.tolist() == [float(kept), float(np.float32(1.0 / kept)),
                               1.0, 0.0]

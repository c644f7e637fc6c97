"""Normalization routing, checked without a GPU: csrc/norm_route.h is pure
host code exposed as ``norm_route(family, rows, C, bf16)``, and the launchers
of norm.hip launch exactly what it returns. tests/test_norm_exact.py asserts
its hand-written route tables against it on the GPU; its CPU emulation uses
the Python model ``route_rows`` / ``route_bn``. Here the two are held equal:
on every table shape, on both sides of every gate, and on a seeded sample."""

import random

import pytest

OPS = pytest.importorskip("baton_amd.ops._hip_ops")

from test_norm_exact import (BF16, BN_KEYS, BN_SHAPES, FP32, KBLOCK, KMAXGRID,
                             ROW_KEYS, ROW_SHAPES, dname, dres_allowed,
                             route_bn, route_rows, vec_width)

DTYPES = (BF16, FP32)


def rows(family, R, C, dt):
    return OPS.norm_route(family, R, C, dt == BF16)


def agree_rows(R, C, dt):
    """norm_route equals the model for both row families; the fields the
    model does not carry follow from the ones it does."""
    want = route_rows(R, C, dt)
    for family in ("ln", "rms"):
        d = rows(family, R, C, dt)
        got = tuple(d[k] for k in ROW_KEYS)
        assert got == want, (family, R, C, dname(dt), got, want)
        assert d["grid"] == min(R, KMAXGRID)
        assert d["chunks"] == -(-C // 64)
        assert d["direct_store"] == (d["grid_y"] == 1)
        assert (d["grid_y"] - 1) * d["rows_per_block"] < R \
            <= d["grid_y"] * d["rows_per_block"]
    return d


def agree_bn(M, C, dt):
    want = route_bn(M, C, dt)
    d = rows("bn", M, C, dt)
    got = tuple(d[k] for k in BN_KEYS)
    assert got == want, (M, C, dname(dt), got, want)
    assert d["chunks"] == -(-C // 64)
    assert d["dres_ok"] == dres_allowed(C, dt) == (d["dx"] == "vec")
    assert d["elem_grid"] == max(1, min(KMAXGRID,
                                        -(-(M * C // 4 + 1) // KBLOCK)))
    assert d["norm_lds"] == (8 * C if d["norm"] == "vec" else 0)
    assert d["dx_lds"] == (12 * C if d["dx"] == "vec" else 0)
    assert (d["grid_y"] - 1) * d["rows_per_block"] < M \
        <= d["grid_y"] * d["rows_per_block"]
    return d


def test_table_shapes():
    for (R, C) in ROW_SHAPES:
        for dt in DTYPES:
            agree_rows(R, C, dt)
    for (M, C), v in BN_SHAPES.items():
        for dt in v[4]:
            agree_bn(M, C, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_row_gates(dt):
    V = vec_width(dt)
    # C % V
    for C in (8, 12, 100):
        assert agree_rows(3, C, dt)["vec"] == (C % V == 0)
    # the second loop trip: C / V = 256, 257 vectors; 256, 257 elements
    assert agree_rows(3, 256 * V, dt)["trips"] == 1
    assert agree_rows(3, 257 * V, dt)["trips"] == 2
    assert agree_rows(3, 255, dt)["trips"] == 1      # odd: element by element
    assert agree_rows(3, 257, dt)["trips"] == 2
    # the grid cap
    d = agree_rows(2048, 64, dt)
    assert (d["grid"], d["capped"]) == (2048, False)
    d = agree_rows(2049, 64, dt)
    assert (d["grid"], d["capped"]) == (2048, True)
    # the rows_per_block floor; grid_y 1 -> 2, direct store -> atomics
    d = agree_rows(128, 64, dt)
    assert (d["rows_per_block"], d["grid_y"], d["direct_store"]) == \
        (128, 1, True)
    d = agree_rows(129, 64, dt)
    assert (d["rows_per_block"], d["grid_y"], d["direct_store"]) == \
        (128, 2, False)
    # above the floor: 1024 / 1 = 1024 target blocks
    d = agree_rows(1024 * 128 + 1, 64, dt)
    assert (d["rows_per_block"], d["grid_y"]) == (129, 1017)
    # chunks > 1024: the target clamps to 1, one row block whatever R
    d = agree_rows(5000, 64 * 1024 + 1, dt)
    assert (d["chunks"], d["rows_per_block"], d["grid_y"]) == (1025, 5000, 1)


@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_bn_gates(dt):
    V = vec_width(dt)
    # C % 64 for the stats kernels
    assert agree_bn(40, 64, dt)["stats"] == "vec"
    assert agree_bn(40, 72, dt)["stats"] == "scalar"
    # C % V for the element passes
    for C in (8, 12, 100):
        d = agree_bn(9, C, dt)
        want = "vec" if C % V == 0 else "scalar"
        assert (d["norm"], d["dx"], d["dres_ok"]) == (want, want, C % V == 0)
    # the rows_per_block floor and grid_y 1 -> 2
    d = agree_bn(64, 64, dt)
    assert (d["rows_per_block"], d["grid_y"]) == (64, 1)
    d = agree_bn(65, 64, dt)
    assert (d["rows_per_block"], d["grid_y"]) == (64, 2)
    d = agree_bn(2048 * 64 + 1, 64, dt)
    assert (d["rows_per_block"], d["grid_y"]) == (65, 2017)
    # the LDS limits: 48 KiB exactly at both, the scalar form one vector on
    d = agree_bn(40, 6144, dt)
    assert (d["norm"], d["norm_lds"]) == ("vec", 49152)
    d = agree_bn(40, 6144 + V, dt)
    assert (d["norm"], d["norm_lds"]) == ("scalar", 0)
    d = agree_bn(40, 4096, dt)
    assert (d["dx"], d["dx_lds"], d["dres_ok"]) == ("vec", 49152, True)
    d = agree_bn(40, 4096 + V, dt)
    assert (d["dx"], d["dx_lds"], d["dres_ok"]) == ("scalar", 0, False)
    # chunks > 2048: the target clamps to 1
    d = agree_bn(300, 64 * 2048 + 1, dt)
    assert (d["chunks"], d["rows_per_block"], d["grid_y"]) == (2049, 300, 1)
    # the element grid: its floor and its cap
    assert agree_bn(1, 1, dt)["elem_grid"] == 1
    assert agree_bn(4093, 512, dt)["elem_grid"] == 2047
    assert agree_bn(4094, 512, dt)["elem_grid"] == 2048
    assert agree_bn(4097, 512, dt)["elem_grid"] == 2048


def test_random_sample():
    rng = random.Random(20261021)
    for _ in range(400):
        R = rng.choice((rng.randint(1, 300), rng.randint(1, 5000),
                        rng.randint(1, 3_000_000)))
        C = rng.choice((rng.randint(1, 130), rng.randint(1, 9000),
                        8 * rng.randint(1, 1200), rng.randint(1, 200_000)))
        dt = rng.choice(DTYPES)
        agree_rows(R, C, dt)
        agree_bn(R, C, dt)


def test_refuses_bad_arguments():
    with pytest.raises(RuntimeError, match="family must be ln, rms or bn"):
        OPS.norm_route("gn", 4, 64, True)
    for R, C in ((0, 64), (4, 0), (4, 2 ** 31)):
        with pytest.raises(RuntimeError, match="bad shape"):
            OPS.norm_route("ln", R, C, True)

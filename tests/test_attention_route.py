"""Attention routing, checked without a GPU: csrc/attn_route.h is pure host
code exposed as ``softmax_route(rows, C, bf16)`` and ``flash_route(B, S, H,
KVH, DH, ...)``; the softmax launchers launch exactly what the first returns,
flash.hip sizes its LDS from the header and its launchers launch the grids of
the second, and flash_fwd / flash_bwd / _flash_eligible refuse from its text.
tests/test_softmax_exact.py asserts its hand-written route table against
softmax_route on the GPU and its Python model ``route`` is held equal to it
here: on every table shape, on both sides of every gate, and on a seeded
sample. flash_route is checked gate by gate."""

import random

import pytest

OPS = pytest.importorskip("baton_amd.ops._hip_ops")

from test_softmax_exact import BF16, FP32, KMAXGRID, SHAPES, route

DTYPES = (BF16, FP32)


def agree_softmax(R, C, dt):
    """softmax_route equals the model; the fields the model does not carry
    follow from the ones it does."""
    d = OPS.softmax_route(R, C, dt == BF16)
    got = (d["kernel"], d["vec"], d["capped"])
    assert got == route(R, C, dt), (R, C, dt, got, route(R, C, dt))
    rows = 4 if d["kernel"] == "wave" else 1
    assert d["rows_per_block"] == rows
    assert d["grid"] == min(KMAXGRID, -(-R // rows))
    return d


def test_softmax_table_shapes():
    for (R, C), (kernel, vec_bf16, vec_fp32, trip) in SHAPES.items():
        for dt in DTYPES:
            d = agree_softmax(R, C, dt)
            assert (d["kernel"], d["vec"], d["capped"]) == \
                (kernel, vec_bf16 if dt == BF16 else vec_fp32, trip)


@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "fp32"))
def test_softmax_gates(dt):
    V = 8 if dt == BF16 else 4
    # wave-per-row up to C = 1024
    assert agree_softmax(9, 1024, dt)["kernel"] == "wave"
    assert agree_softmax(9, 1025, dt)["kernel"] == "block"
    # 16-byte vectors from 64 of them on, and only whole ones
    assert not agree_softmax(9, 64 * V - V, dt)["vec"]
    assert agree_softmax(9, 64 * V, dt)["vec"]
    assert not agree_softmax(9, 64 * V + 1, dt)["vec"]
    # the grid cap: 2048 blocks of 4 rows (wave) or of one row (block)
    d = agree_softmax(8192, 64, dt)
    assert (d["grid"], d["capped"]) == (2048, False)
    d = agree_softmax(8193, 64, dt)
    assert (d["grid"], d["capped"]) == (2048, True)
    d = agree_softmax(2048, 1032, dt)
    assert (d["grid"], d["capped"]) == (2048, False)
    d = agree_softmax(2049, 1032, dt)
    assert (d["grid"], d["capped"]) == (2048, True)
    assert agree_softmax(7, 64, dt)["grid"] == 2


def test_softmax_random_sample():
    rng = random.Random(20261021)
    for _ in range(400):
        R = rng.choice((rng.randint(1, 300), rng.randint(1, 10_000),
                        rng.randint(1, 3_000_000)))
        C = rng.choice((rng.randint(1, 130), rng.randint(1, 2100),
                        8 * rng.randint(1, 300), rng.randint(1, 200_000)))
        agree_softmax(R, C, rng.choice(DTYPES))


def test_softmax_refuses_bad_shape():
    for R, C in ((0, 64), (4, 0), (4, 2 ** 31)):
        with pytest.raises(RuntimeError, match="bad shape"):
            OPS.softmax_route(R, C, True)


# ---- flash -------------------------------------------------------------------

VIEWS_FWD = ("q", "k", "v", "o")
VIEWS_BWD = VIEWS_FWD + ("dout", "dq", "dk", "dv")


def flash(B=2, S=64, H=4, KVH=2, DH=64, **kw):
    return OPS.flash_route(B, S, H, KVH, DH, **kw)


def contiguous(S, heads, DH):
    return [S * heads * DH, heads * DH, DH, 1, 0]


def refused(d, *words):
    assert not d["eligible"]
    for w in words:
        assert w in d["refusal"], (w, d["refusal"])


@pytest.mark.parametrize("DH", (32, 64, 128))
def test_flash_eligible_grids_and_lds(DH):
    for causal in (False, True):
        for varlen in (False, True):
            for bwd in (False, True):
                d = flash(DH=DH, causal=causal, varlen=varlen, bwd=bwd)
                assert d["eligible"] and d["refusal"] is None
    B, H = 3, 6
    for S in (1, 127, 128, 129, 257):
        d = flash(B=B, S=S, H=H, KVH=2, DH=DH, bwd=True)
        assert d["eligible"]
        tiles = (-(-S // 128), B * H)
        assert d["grid_fwd"] == d["grid_dq"] == d["grid_dkv"] == tiles
        assert d["grid_delta"] == (-(-S // 4), B * H)
        assert (d["lds_fwd"], d["lds_dq"], d["lds_dkv"]) == \
            (512 * DH, 384 * DH, 768 * DH)
        assert d["G"] == 3
    assert flash(H=4, KVH=4, DH=DH)["G"] == 1
    assert flash(H=4, KVH=1, DH=DH)["G"] == 4


def test_flash_refuses_head_dim_dtype_and_heads():
    for DH in (16, 48, 256):
        refused(flash(DH=DH), "unsupported head_dim", str(DH))
    refused(flash(bf16=False), "q must be a bf16 GPU tensor")
    refused(flash(H=3, KVH=2), "q heads must be a multiple of kv heads")
    refused(flash(H=4, KVH=0), "q heads must be a multiple of kv heads")


@pytest.mark.parametrize("bwd", (False, True), ids=("fwd", "bwd"))
def test_flash_refuses_each_view(bwd):
    S, H, KVH, DH = 64, 4, 2, 64
    for name in (VIEWS_BWD if bwd else VIEWS_FWD):
        heads = KVH if name in ("k", "v") else H
        ok = contiguous(S, heads, DH)
        assert flash(S=S, H=H, KVH=KVH, DH=DH, bwd=bwd,
                     views={name: ok})["eligible"]

        def bad(i, value):
            v = list(ok)
            v[i] = value
            return flash(S=S, H=H, KVH=KVH, DH=DH, bwd=bwd, views={name: v})

        refused(bad(3, 2), name + " head_dim must be contiguous")
        refused(bad(4, 8), name + " must start on a 16-byte boundary")
        for i in range(3):
            refused(bad(i, ok[i] + 4), name + " strides must be multiples of 8")
            assert bad(i, ok[i] + 8)["eligible"]
    if not bwd:   # the backward's views are not looked at by the forward
        assert flash(views={"dq": [1, 1, 1, 2, 8]})["eligible"]


def test_flash_route_refuses_bad_arguments():
    for kw in (dict(B=0), dict(S=0), dict(H=0), dict(DH=0), dict(KVH=-1)):
        with pytest.raises(RuntimeError, match="bad shape"):
            flash(**kw)
    with pytest.raises(RuntimeError):   # a view is 4 strides and the base
        flash(views={"q": [1, 2, 3]})

"""GEMM routing, checked without a GPU: the planner (csrc/gemm_plan.h) is
pure host code exposed as ``gemm_plan(...)``, so which kernel, tile, grid and
K split a shape gets is asserted here instead of being inferred from numerics
that pass whichever kernel runs.

Expectations were derived by hand from the routing rules, not printed from
the planner. All problems are bf16, alpha 1, beta 0, no bias / relu unless
the row says otherwise."""

import pytest

OPS = pytest.importorskip("baton_amd.ops._hip_ops")

NT, NN, TN = 0, 1, 2


def plan(M, N, K, layout=NT, **kw):
    return OPS.gemm_plan(M, N, K, layout=layout, **kw)


def check(got, want):
    for key, val in want.items():
        assert got[key] == val, f"{key}: got {got[key]!r}, want {val!r} in {got}"


NO_T = dict(transpose_a=False, transpose_b=False)

TABLE = [
    # dense G9: 16 x 10 = 160 blocks, exactly the gate; operands L3-resident
    ((4096, 2560, 512, NT), {},
     dict(kind="G9", layout=NT, tile=(256, 256), grid=(10, 16, 1), use_swz=0,
          m_main=4096, remainder=None, **NO_T)),
    ((4096, 2560, 512, NT), dict(has_bias=True),
     dict(kind="G9", grid=(10, 16, 1), use_swz=0, remainder=None, **NO_T)),
    # 15 x 10 = 150 blocks: below the gate
    ((3840, 2560, 512, NT), {}, dict(kind="TwoPhase", tile=(128, 128))),
    # K not a multiple of the g9 K-tile
    ((4096, 2560, 480, NT), {}, dict(kind="TwoPhase", tile=(128, 128))),
    ((256, 256, 64, NT), {},
     dict(kind="TwoPhase", tile=(128, 64), grid=(4, 2, 1), use_swz=0,
          m_main=256, remainder=None)),
    ((1024, 512, 4096, NT), {},
     dict(kind="G9Slab", splits=16, k_chunk=256, grid=(2, 4, 16), use_swz=1)),
    ((2000, 512, 1024, NT), {},
     dict(kind="TwoPhaseSplitK", tile=(128, 128), splits=8, k_chunk=128,
          grid=(4, 16, 8), use_swz=0)),
    # ragged M: 10 x 16 = 160 G9 blocks on 2560 rows, 48 rows left over
    ((2608, 4096, 192, NT), {},
     dict(kind="G9", m_main=2560, grid=(16, 10, 1), use_swz=0, **NO_T)),
    # the same behind the big-B NN re-layout: the remainder is NT too
    ((2608, 4096, 192, NN), {},
     dict(kind="G9", m_main=2560, layout=NT, transpose_a=False,
          transpose_b=True)),
    ((768, 768, 16384, TN), {},
     dict(kind="G9Slab", layout=NT, transpose_a=True, transpose_b=True,
          splits=32, k_chunk=512, grid=(3, 3, 32), use_swz=1)),
    ((256, 256, 1152, NT), {},
     dict(kind="G8Slab", splits=4, k_chunk=288, grid=(1, 1, 4), use_swz=1)),
    # k_chunk 320 = 5 K-tiles: the g9 odd-parity tail
    ((256, 256, 1280, NT), {},
     dict(kind="G9Slab", splits=4, k_chunk=320, grid=(1, 1, 4), use_swz=1)),
    ((2048, 16, 4096, NT), {},
     dict(kind="TwoPhaseSplitK", tile=(128, 32), splits=32, k_chunk=128,
          grid=(1, 16, 32), **NO_T)),
    # B is 128 KiB, under the 1 MiB re-layout threshold
    ((2048, 16, 4096, NN), {},
     dict(kind="TwoPhaseSplitK", layout=NN, tile=(128, 32), splits=32,
          k_chunk=128, **NO_T)),
    # slab count stops at 2 (K % 4 != 0) and 15261 is no multiple of 32
    ((4096, 768, 30522, NN), {},
     dict(kind="TwoPhaseSplitK", layout=NT, transpose_a=False,
          transpose_b=True, tile=(128, 128), splits=2, k_chunk=15264,
          grid=(6, 32, 2), use_swz=0)),
    ((1024, 512, 4096, NT), dict(beta=1.0), dict(kind="TwoPhase")),
    ((4096, 2560, 512, NT), dict(beta=1.0), dict(kind="TwoPhase")),
    ((4096, 2560, 512, NT), dict(relu=True), dict(kind="TwoPhase")),
    ((1024, 512, 4096, NT), dict(alpha=0.5),
     dict(kind="TwoPhase", tile=(128, 64))),
    ((1024, 512, 4096, NT), dict(bf16=False),
     dict(kind="TwoPhaseSplitK", tile=(128, 128), splits=16, k_chunk=256)),
    # TN stays native with out_f32 or `direct`; NN stays native with `direct`
    ((768, 768, 4096, TN), dict(out_f32=True),
     dict(kind="TwoPhaseSplitK", layout=TN, **NO_T)),
    ((768, 768, 4096, TN), dict(direct=True),
     dict(kind="TwoPhaseSplitK", layout=TN, **NO_T)),
    ((4096, 768, 30522, NN), dict(direct=True),
     dict(kind="TwoPhaseSplitK", layout=NN, **NO_T)),
]


@pytest.mark.parametrize("shape,kw,want", TABLE)
def test_plan_table(shape, kw, want):
    M, N, K, layout = shape
    check(plan(M, N, K, layout, **kw), want)


def test_plan_ragged_remainder():
    """The rows a ragged-M G9 plan leaves over get a plan of their own: what
    a fresh 48-row NT problem gets (64x128 tiles, N > M)."""
    got = plan(2608, 4096, 192)
    want = dict(kind="TwoPhase", layout=NT, tile=(64, 128), grid=(32, 1, 1),
                use_swz=0, m_main=48)
    check(got["remainder"], want)
    check(plan(2608, 4096, 192, NN)["remainder"], want)
    check(plan(48, 4096, 192), want)


# benchmarks/gemm_bench.py shapes. Every B there is >= 1 MiB, so NN
# transposes B and TN transposes both: all three layouts run the NT plan.
BENCH = [
    ("square-4k", 4096, 4096, 4096,
     dict(kind="G9", grid=(16, 16, 1), use_swz=0)),
    ("bert-qkv", 4096, 2304, 768,           # 16 x 9 = 144 blocks < 160
     dict(kind="TwoPhase", tile=(128, 128), grid=(18, 32, 1), use_swz=0)),
    ("bert-fc1", 4096, 3072, 768,
     dict(kind="G9", grid=(12, 16, 1), use_swz=0)),
    ("bert-fc2-dgrad", 4096, 768, 3072,     # 192 tiles of 128^2, 48 of 256^2
     dict(kind="G9Slab", splits=8, k_chunk=384, grid=(3, 16, 8), use_swz=1)),
    ("llama-gate", 2048, 14336, 4096,       # operands 128 MiB
     dict(kind="G9", grid=(56, 8, 1), use_swz=0)),
    ("llama-down", 2048, 4096, 14336,       # 8 x 16 = 128 blocks; 168 MiB
     dict(kind="TwoPhase", tile=(128, 128), grid=(32, 16, 1), use_swz=0)),
    ("wgrad-768", 768, 2304, 4096,
     dict(kind="G9Slab", splits=8, k_chunk=512, grid=(9, 3, 8), use_swz=1)),
    ("llama-q16", 8192, 4096, 4096,
     dict(kind="G9", grid=(16, 32, 1), use_swz=0)),
    ("llama-kv16", 8192, 1024, 4096,        # 32 x 4 = 128 blocks
     dict(kind="TwoPhase", tile=(128, 128), grid=(8, 64, 1), use_swz=0)),
    ("llama-gate16", 8192, 14336, 4096,     # operands 176 MiB
     dict(kind="G9", grid=(56, 32, 1), use_swz=0)),
    ("llama-down16", 8192, 4096, 14336,     # operands 336 MiB
     dict(kind="G9", grid=(16, 32, 1), use_swz=1)),
    ("llama-head16", 8192, 128256, 4096,
     dict(kind="G9", grid=(501, 32, 1), use_swz=1)),
    ("bert-wg-qkv", 2304, 768, 16384,
     dict(kind="G9Slab", splits=8, k_chunk=2048, grid=(3, 9, 8), use_swz=1)),
    ("bert-wg-fc1", 3072, 768, 16384,
     dict(kind="G9Slab", splits=8, k_chunk=2048, grid=(3, 12, 8), use_swz=1)),
    ("bert-wg-fc2", 768, 3072, 16384,
     dict(kind="G9Slab", splits=8, k_chunk=2048, grid=(12, 3, 8), use_swz=1)),
]


@pytest.mark.parametrize("name,M,N,K,want", BENCH, ids=[b[0] for b in BENCH])
@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_plan_bench_shapes(name, M, N, K, want, layout):
    got = plan(M, N, K, layout)
    check(got, dict(want, layout=NT, m_main=M, remainder=None,
                    transpose_a=layout == TN, transpose_b=layout != NT))


def test_plan_batched_entry_points():
    """gemm_batched / bmm_strided never re-lay-out or split K, and only an
    unbatched, unstrided call may take G9."""
    # attention scores: 96 batches of 512x512x64 -> 16 tiles each, 1536 total
    check(plan(512, 512, 64, NT, nbatch=96, batched=True),
          dict(kind="TwoPhase", tile=(128, 128), grid=(4, 4, 96), **NO_T))
    # few batches: 2 x 16 tiles < 384 -> narrow tile
    check(plan(512, 512, 64, NT, nbatch=2, batched=True),
          dict(kind="TwoPhase", tile=(128, 64), grid=(8, 4, 2)))
    # long K, small grid: gemm() would split, the batched entry does not
    check(plan(1024, 512, 4096, NT, batched=True),
          dict(kind="TwoPhase", tile=(128, 64), splits=1))
    check(plan(4096, 2560, 512, NT, batched=True), dict(kind="G9"))
    check(plan(4096, 2560, 512, NT, batched=True, strided=True),
          dict(kind="TwoPhase"))
    check(plan(4096, 2560, 512, NT, batched=True, nbatch=2),
          dict(kind="TwoPhase"))

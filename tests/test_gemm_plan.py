"""GEMM routing, checked without a GPU: the planner (csrc/gemm_plan.h) is
pure host code exposed as ``gemm_plan(...)``, so which kernel, tile, grid and
K split a shape gets is asserted here instead of being inferred from numerics
that pass whichever kernel runs.

Expectations were derived by hand from the routing rules, not printed from
the planner. All problems are bf16, alpha 1, beta 0, no bias / relu unless
the row says otherwise.

Below the tables: the combinations no kernel exists for must raise, and a
seeded sample of problems is checked against the launchers' preconditions.
tests/test_gemm_exact.py checks on a GPU what the planned kernels compute."""

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


# ---- combinations without a kernel -----------------------------------------
# The dense launch ladder has the fp32-output bf16 kernel for TN only and the
# relu epilogue for NT only; gemm_unsupported() (gemm_plan.h) refuses the
# rest, here and in gemm() / gemm_batched() / bmm_strided().

@pytest.mark.parametrize("layout,kw", [
    (NT, dict(out_f32=True)),
    (NN, dict(out_f32=True)),
    (NN, dict(relu=True)),
    (TN, dict(relu=True)),
    (NN, dict(relu=True, bf16=False)),
    (NT, dict(out_f32=True, batched=True, nbatch=6)),
    (NN, dict(out_f32=True, batched=True, nbatch=6)),
    # G9-sized: out_f32 keeps it off G9, and the 2-phase NT has no fp32 out
    (NT, dict(out_f32=True, M=4096, N=2560, K=512)),
    # alpha != 1 takes a long-K shape off the split routes
    (NT, dict(out_f32=True, alpha=0.5, M=136, N=72, K=1040)),
])
def test_plan_refuses_unsupported(layout, kw):
    kw = dict(kw)
    M, N, K = kw.pop("M", 200), kw.pop("N", 136), kw.pop("K", 104)
    with pytest.raises(RuntimeError, match="unsupported"):
        plan(M, N, K, layout, **kw)


def test_plan_keeps_supported_neighbours():
    """What sits next to the refused combinations keeps planning."""
    # the split routes accumulate in fp32 whatever the layout
    check(plan(136, 72, 1040, NT, out_f32=True), dict(kind="TwoPhaseSplitK"))
    check(plan(136, 72, 1040, NN, out_f32=True), dict(kind="TwoPhaseSplitK"))
    check(plan(256, 256, 1024, NT, out_f32=True), dict(kind="G9Slab"))
    # native TN has the fp32-output kernel, batched too
    check(plan(200, 136, 104, TN, out_f32=True),
          dict(kind="TwoPhase", layout=TN))
    check(plan(128, 64, 104, TN, out_f32=True, batched=True, nbatch=6),
          dict(kind="TwoPhase", layout=TN))
    # with fp32 inputs out_f32 changes nothing
    check(plan(200, 136, 104, NT, out_f32=True, bf16=False),
          dict(kind="TwoPhase"))
    check(plan(200, 136, 104, NT, relu=True), dict(kind="TwoPhase"))


# ---- launcher preconditions over a sample of problems ------------------------
# The launchers refuse (a hard error at run time) a plan that does not tile
# its problem. Their conditions, restated from launch_gemm_2ph,
# launch_gemm_2ph_splitk, launch_gemm_nt_g9 and launch_gemm_nt_slab, are
# asserted here for a seeded sample of problems instead.

TILES = {(128, 128), (128, 64), (64, 128), (128, 32)}


def cdiv(a, b):
    return -(-a // b)


def draw_dim(rng, hi):
    """Biased toward multiples of 32, 64 and 256 and their neighbours."""
    step = rng.choice([1, 32, 32, 64, 64, 256, 256, 256])
    if step == 1:
        return rng.randint(1, hi)
    v = step * rng.randint(1, hi // step) + rng.choice([-1, 0, 0, 0, 0, 1])
    return min(max(v, 1), hi)


def draw_problem(rng):
    slab_shaped = rng.random() < 0.2
    if slab_shaped:
        # few 256-tiles, K a whole number of 32-wide k-halves
        M, N = 256 * rng.randint(1, 8), 256 * rng.randint(1, 8)
        K = 32 * rng.randint(16, 625)
    else:
        M, N, K = draw_dim(rng, 5000), draw_dim(rng, 5000), draw_dim(rng, 20000)
    # the split routes and the re-layouts need a plain problem
    plain = slab_shaped or rng.random() < 0.4
    batched = not slab_shaped and rng.random() < 0.25
    return dict(
        M=M, N=N, K=K,
        layout=rng.choice([NT, NN, TN]), bf16=rng.random() < 0.7,
        out_f32=rng.random() < 0.15,
        has_bias=not plain and rng.random() < 0.5,
        relu=not plain and rng.random() < 0.3,
        alpha=1.0 if plain else rng.choice([1.0, 0.5, 2.0, -1.5]),
        beta=0.0 if plain else rng.choice([0.0, 1.0, 0.5]),
        direct=rng.random() < 0.25, batched=batched,
        nbatch=rng.choice([1, 2, 6, 96]) if batched else 1,
        strided=batched and rng.random() < 0.5)


def is_plain(p):
    return p["beta"] == 0.0 and not p["has_bias"] and not p["relu"]


def takes_split_route(p):
    """gemm() splits K for plain alpha-1 problems with a small tile grid and
    a long contraction; the batched entry points never do."""
    tiles = cdiv(p["M"], 128) * cdiv(p["N"], 32 if p["N"] <= 32 else 128)
    return (not p["batched"] and is_plain(p) and p["alpha"] == 1.0 and
            tiles < 256 and p["K"] >= 1024)


def is_refused(p):
    # relu is not plain, so no re-layout: the effective layout is p's own.
    # out_f32 keeps TN native, and NT / NN never become TN.
    if p["relu"] and p["layout"] != NT:
        return True
    return (p["out_f32"] and p["bf16"] and p["layout"] != TN and
            not takes_split_route(p))


def check_two_phase(d, M, N, gz):
    bm, bn = d["tile"]
    assert d["tile"] in TILES
    assert d["grid"] == (cdiv(N, bn), cdiv(M, bm), gz)


def check_launchable(p, d):
    M, N, K = p["M"], p["N"], p["K"]
    kind = d["kind"]
    relaid = d["transpose_a"] or d["transpose_b"]
    assert d["layout"] == (NT if relaid else p["layout"])
    if relaid:
        assert is_plain(p) and not p["direct"] and not p["batched"]
    if kind != "G9":
        assert d["m_main"] == M and d["remainder"] is None
    if kind == "TwoPhase":
        check_two_phase(d, M, N, p["nbatch"])
        assert d["splits"] == 1
        return
    if kind == "G9":
        assert p["bf16"] and not p["out_f32"] and d["layout"] == NT
        assert not p["relu"] and p["beta"] == 0.0
        assert p["nbatch"] == 1 and not p["strided"]
        assert N % 256 == 0 and K % 64 == 0 and K >= 64
        m_main = d["m_main"]
        assert 0 < m_main <= M and m_main % 256 == 0 and M - m_main < 256
        assert d["tile"] == (256, 256)
        assert d["grid"] == (N // 256, m_main // 256, 1)
        rem = d["remainder"]
        assert (rem is not None) == (m_main < M)
        if rem is not None:
            assert rem["kind"] == "TwoPhase" and rem["layout"] == NT
            assert rem["m_main"] == M - m_main and rem["splits"] == 1
            check_two_phase(rem, M - m_main, N, 1)
        return
    # the split routes: gemm() only, plain, alpha 1
    assert takes_split_route(p)
    splits, k_chunk = d["splits"], d["k_chunk"]
    assert splits >= 1
    if kind == "TwoPhaseSplitK":
        check_two_phase(d, M, N, splits)
        assert k_chunk >= 32 and k_chunk % 32 == 0
        assert splits * k_chunk >= K > (splits - 1) * k_chunk
        return
    assert kind in ("G9Slab", "G8Slab")
    assert p["bf16"] and d["layout"] == NT
    assert M % 256 == 0 and N % 256 == 0
    assert d["tile"] == (256, 256)
    assert d["grid"] == (N // 256, M // 256, splits)
    assert splits * k_chunk == K and k_chunk >= 64
    assert k_chunk % (64 if kind == "G9Slab" else 32) == 0


def test_plan_sweep_launcher_preconditions():
    import random

    rng = random.Random(20240611)
    kinds, refused = {}, 0
    for _ in range(2000):
        p = draw_problem(rng)
        args = (p["M"], p["N"], p["K"], p["layout"])
        kw = {k: v for k, v in p.items() if k not in ("M", "N", "K", "layout")}
        if is_refused(p):
            refused += 1
            with pytest.raises(RuntimeError, match="unsupported"):
                plan(*args, **kw)
            continue
        d = plan(*args, **kw)
        try:
            check_launchable(p, d)
        except AssertionError as e:
            raise AssertionError(f"{p} -> {d}: {e}") from e
        kinds[d["kind"]] = kinds.get(d["kind"], 0) + 1
    print(f"sweep: {kinds}, {refused} refused")
    # the sample reaches every route
    assert set(kinds) == {"TwoPhase", "TwoPhaseSplitK", "G9", "G9Slab",
                          "G8Slab"}
    assert refused > 50

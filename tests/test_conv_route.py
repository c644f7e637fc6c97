"""Conv routing, checked without a GPU: the router (csrc/conv_route.h) is
pure host code exposed as ``conv_route(op, N, H, W, Cin, Cout, KH, KW,
stride, pad, bf16=True)``, so which kernel, tile, grid and pixel split a
convolution gets is asserted here instead of being inferred from numerics
that pass whichever kernel runs.

Expectations were derived by hand from the routing rules, not printed from
the router:

fwd / dgrad (rows M = N HO WO / N H W; columns = Cout / Cin; contracted
channels kc = Cin / Cout), first match wins:
  Halo     bf16, 3x3 s1 p1, 128 % W == 0, H W % 128 == 0, kc % 32 == 0,
           columns % 64 == 0; grid (M / 128, columns / 64)
  Conv8    bf16, dgrad stride 1, columns % 256 == 0, kc % 32 == 0,
           KH KW kc % 64 == 0, ceil(M / 256) * columns / 256 >= 256;
           grid (columns / 256, ceil(M / 256))
  DgradPhase  dgrad, stride 2, Cout % 32 == 0; generic tile; grid = (sum of
           the four parity classes' ceil(rows / 128)) * column tiles
  Generic  tile 128 x (64 if columns <= 64 else 128), fast = kc % 32 == 0
wgrad (P = N HO WO):
  WgradPx  wgpx::eligible (tests/test_wgrad_px_map.py)
  Wgrad1x1Slab / Wgrad1x1SplitK  1x1 s1 p0: the GEMM planner's slab route
           when bf16, Cin and Cout % 256 == 0 and slab_splits > 1
  WgradGeneric  the rest; see tests/test_conv_exact.py for the split rule

tests/test_conv_exact.py checks on a GPU what the routed kernels compute;
its case table carries each case's expected route and is asserted here too."""

import random

import pytest

from test_conv_exact import BF16, CASES, out_hw

OPS = pytest.importorskip("baton_amd.ops._hip_ops")


def route(op, N, H, W, Cin, Cout, K, s, p, bf16=True):
    KH, KW = (K, K) if isinstance(K, int) else K
    return OPS.conv_route(op, N, H, W, Cin, Cout, KH, KW, s, p, bf16=bf16)


def check(got, want, what=""):
    for key, val in want.items():
        assert got[key] == val, \
            f"{what}: {key} is {got[key]!r}, want {val!r} in {got}"


@pytest.mark.parametrize("name", list(CASES))
def test_exact_cases_route(name):
    """Every shape tests/test_conv_exact.py runs gets the route it names."""
    c = CASES[name]
    got = OPS.conv_route(c["op"], c["N"], c["H"], c["W"], c["Cin"], c["Cout"],
                         c["KH"], c["KW"], c["s"], c["p"],
                         bf16=c["dtype"] is BF16)
    assert got["out_hw"] == out_hw(c)
    check(got, c["route"], name)


def halo(gx, gy):
    return dict(kind="Halo", tile=(128, 64), grid=(gx, gy, 1))


def c8(gx, gy):
    return dict(kind="Conv8", tile=(256, 256), grid=(gx, gy, 1), use_swz=1)


def gen(bn, gx, gy, fast=True):
    return dict(kind="Generic", tile=(128, bn), grid=(gx, gy, 1), fast=fast)


def phase(bn, gx):
    return dict(kind="DgradPhase", tile=(128, bn), grid=(gx, 1, 1))


def px(gx, gy, splits):     # 16 k-steps of 32 pixels per slice throughout
    return dict(kind="WgradPx", tile=(64, 64), grid=(gx, gy, splits),
                splits=splits, p_chunk=512, transpose_dy=False)


def wg(bm, gx, gy, splits, p_chunk):
    return dict(kind="WgradGeneric", tile=(bm, 128), grid=(gx, gy, splits),
                splits=splits, p_chunk=p_chunk, transpose_dy=True)


SPLITK = dict(kind="Wgrad1x1SplitK", gemm_kind="TwoPhaseSplitK",
              transpose_dy=True, transpose_x=False)


def slab(gx, gy, splits, p_chunk):
    return dict(kind="Wgrad1x1Slab", gemm_kind="G9Slab", tile=(256, 256),
                grid=(gx, gy, splits), splits=splits, p_chunk=p_chunk,
                transpose_dy=True, transpose_x=True, use_swz=1)


# Every conv of ResNet-18 / ResNet-50 as models/resnet.py builds them for
# 32x32 input (pad = K // 2), bf16, batch 256: rows per resolution 32 / 16 /
# 8 / 4 are 262144 / 65536 / 16384 / 4096, i.e. 1024 / 256 / 64 / 16 tiles of
# 256. (Cin, Cout, K, stride, H): (fwd, dgrad, wgrad)
RESNET_N = 256
RESNET = {
    # ---- ResNet-18 ----
    # stem
    (3, 64, 3, 1, 32): (gen(64, 1, 2048, fast=False), gen(64, 1, 2048),
                        wg(64, 1, 1, 512, 512)),
    (64, 64, 3, 1, 32): (halo(2048, 1), halo(2048, 1), px(1, 1, 512)),
    # 3x3 s2: 576 columns = 5 tiles -> 102 slices wanted of 65536 pixels ->
    # 643 -> 672 per slice, 98 slices
    (64, 128, 3, 2, 32): (gen(128, 1, 512), phase(64, 2048),
                          wg(128, 5, 1, 98, 672)),
    (128, 128, 3, 1, 16): (halo(512, 2), halo(512, 2), px(2, 2, 128)),
    (64, 128, 1, 2, 32): (gen(128, 1, 512), phase(64, 2048),
                          wg(128, 1, 1, 512, 128)),
    # 64 row tiles x 1 column tile: below the conv8 gate at this batch
    (128, 256, 3, 2, 16): (gen(128, 2, 128), phase(128, 512),
                           wg(128, 9, 2, 27, 608)),
    (256, 256, 3, 1, 8): (gen(128, 2, 128), gen(128, 2, 128), px(4, 4, 32)),
    (128, 256, 1, 2, 16): (gen(128, 2, 128), phase(128, 512),
                           wg(128, 1, 2, 256, 64)),
    (256, 512, 3, 2, 8): (gen(128, 4, 32), phase(128, 256),
                          wg(128, 18, 4, 7, 608)),
    (512, 512, 3, 1, 4): (gen(128, 4, 32), gen(128, 4, 32), px(8, 8, 8)),
    (256, 512, 1, 2, 8): (gen(128, 4, 32), phase(128, 256),
                          wg(128, 2, 4, 64, 64)),
    # ---- ResNet-50 bottlenecks (3x3 s1 64 @32, 128 @16, 256 @8, 512 @4 as
    # above) ----
    (64, 64, 1, 1, 32): (gen(64, 1, 2048), gen(64, 1, 2048), SPLITK),
    (256, 64, 1, 1, 32): (gen(64, 1, 2048), c8(1, 1024), SPLITK),
    (64, 256, 1, 1, 32): (c8(1, 1024), gen(64, 1, 2048), SPLITK),
    (256, 128, 1, 1, 32): (gen(128, 1, 2048), c8(1, 1024), SPLITK),
    (128, 128, 3, 2, 32): (gen(128, 1, 512), phase(128, 2048),
                           dict(kind="WgradGeneric", tile=(128, 128))),
    (128, 512, 1, 1, 16): (c8(2, 256), gen(128, 1, 512), SPLITK),
    (256, 512, 1, 2, 32): (c8(2, 256), phase(128, 4096),
                           dict(kind="WgradGeneric", tile=(128, 128))),
    (512, 128, 1, 1, 16): (gen(128, 1, 512), c8(2, 256), SPLITK),
    # exactly 256 blocks forward; wgrad: 2 slab tiles -> 128 slices (256
    # blocks <= 384) of 512 pixels
    (512, 256, 1, 1, 16): (c8(1, 256), c8(2, 256), slab(2, 1, 128, 512)),
    (256, 256, 3, 2, 16): (gen(128, 2, 128), phase(128, 1024),
                           dict(kind="WgradGeneric", tile=(128, 128))),
    (256, 1024, 1, 1, 8): (c8(4, 64), gen(128, 2, 128), slab(1, 4, 64, 256)),
    (512, 1024, 1, 2, 16): (c8(4, 64), phase(128, 2048),
                            dict(kind="WgradGeneric", tile=(128, 128))),
    (1024, 256, 1, 1, 8): (gen(128, 2, 128), c8(4, 64), slab(4, 1, 64, 256)),
    # 64 x 2 = 128 blocks forward, 64 x 4 = 256 backward
    (1024, 512, 1, 1, 8): (gen(128, 4, 128), c8(4, 64), slab(4, 2, 32, 512)),
    (512, 512, 3, 2, 8): (gen(128, 4, 32), phase(128, 512),
                          dict(kind="WgradGeneric", tile=(128, 128))),
    (512, 2048, 1, 1, 4): (gen(128, 16, 32), gen(128, 4, 32),
                           slab(2, 8, 16, 256)),
    (1024, 2048, 1, 2, 8): (gen(128, 16, 32), phase(128, 1024),
                            dict(kind="WgradGeneric", tile=(128, 128))),
    (2048, 512, 1, 1, 4): (gen(128, 4, 32), gen(128, 16, 32),
                           slab(8, 2, 16, 256)),
}


@pytest.mark.parametrize("shape", list(RESNET))
def test_resnet_routes(shape):
    Cin, Cout, K, s, H = shape
    for op, want in zip(("fwd", "dgrad", "wgrad"), RESNET[shape]):
        got = route(op, RESNET_N, H, H, Cin, Cout, K, s, K // 2)
        check(got, want, f"{op} {shape}")


def test_resnet_table_is_complete():
    """The table above lists every conv the two models build."""
    torch = pytest.importorskip("torch")
    from baton_amd.models.resnet import resnet18, resnet50
    from baton_amd.ops.modules import BatonConv2d

    seen = set()
    for model in (resnet18(), resnet50()):
        convs = {}

        def note(mod, args):
            convs.setdefault(mod, args[0].shape[1])

        hooks = [m.register_forward_pre_hook(note) for m in model.modules()
                 if isinstance(m, BatonConv2d)]
        model(torch.randn(2, 32, 32, 3))     # the CPU path of the op layer
        for h in hooks:
            h.remove()
        for mod, H in convs.items():
            w = mod.weight
            assert mod.padding == mod.kernel_size // 2
            seen.add((w.shape[3], w.shape[0], w.shape[1], mod.stride, H))
    assert seen == set(RESNET)


# One shape on each side of each gate that tests/test_conv_exact.py does not
# already sit on. (op, N, H, W, Cin, Cout, K, s, p, bf16) -> expectation
GATES = [
    # conv8 blocks: 4096 x 16 px = 256 row tiles x 2 column tiles; at batch
    # 2040 it is 255 x 1 for Cout 256
    (("fwd", 4096, 4, 4, 512, 512, 3, 1, 1, True), c8(2, 256)),
    (("fwd", 4080, 4, 4, 512, 256, 3, 1, 1, True), gen(128, 2, 510)),
    (("fwd", 4096, 4, 4, 512, 256, 3, 1, 1, True), c8(1, 256)),
    (("fwd", 4096, 4, 4, 512, 256, 3, 1, 1, False), gen(128, 2, 512)),
    # Cout = 384 is no multiple of 256; Cin = 48 no multiple of 32
    (("fwd", 4096, 4, 4, 512, 384, 3, 1, 1, True), gen(128, 3, 512)),
    (("fwd", 4096, 4, 4, 48, 256, 3, 1, 1, True),
     gen(128, 2, 512, fast=False)),
    # 3x3 x 96 = 864 = 13.5 x 64
    (("fwd", 4096, 4, 4, 96, 256, 3, 1, 1, True), gen(128, 2, 512)),
    # conv8 dgrad is stride 1 only: stride 2 goes to the phase kernel (4
    # classes x 4096 x 2 x 2 rows = 128 tiles each, 2 column tiles), stride 3
    # to the generic one
    (("dgrad", 4096, 4, 4, 256, 512, 3, 1, 1, True), c8(1, 256)),
    (("dgrad", 4096, 4, 4, 256, 512, 3, 2, 1, True), phase(128, 1024)),
    (("dgrad", 4096, 4, 4, 256, 512, 3, 3, 1, True), gen(128, 2, 512)),
    # phase kernel: Cout % 32, bf16 or fp32
    (("dgrad", 2, 8, 8, 64, 48, 3, 2, 1, True), gen(64, 1, 1, fast=False)),
    (("dgrad", 2, 8, 8, 64, 64, 3, 2, 1, False), phase(64, 4)),
    # halo before conv8: 16x16 x 256 channels would fit both
    (("fwd", 1024, 16, 16, 256, 256, 3, 1, 1, True), halo(2048, 4)),
    (("dgrad", 1024, 16, 16, 256, 256, 3, 1, 1, True), halo(2048, 4)),
    # halo: W = 2 and W = 256
    (("fwd", 1, 64, 2, 32, 64, 3, 1, 1, True), halo(1, 1)),
    (("fwd", 1, 1, 256, 32, 64, 3, 1, 1, True), gen(64, 1, 2)),
    # generic tile: 64 columns narrow, 65 wide
    (("fwd", 1, 8, 8, 32, 65, 3, 1, 1, True), gen(128, 1, 1)),
    (("dgrad", 1, 8, 8, 65, 32, 3, 1, 1, True), gen(128, 1, 1)),
    # XCD remap flag: activations (2 bytes each) past 200 MiB. 8192 x 32 x 32
    # x (64 + 64) x 2 = 2 GiB; at batch 512 it is 128 MiB
    (("fwd", 8192, 32, 32, 64, 64, 3, 1, 1, False),
     dict(kind="Generic", use_swz=1)),
    (("fwd", 512, 32, 32, 64, 64, 3, 1, 1, False),
     dict(kind="Generic", use_swz=0)),
    # pixel-major wgrad: W = 12 and fp32 are out
    (("wgrad", 2, 8, 8, 64, 64, 3, 1, 1, True), px(1, 1, 4) | dict(p_chunk=32)),
    (("wgrad", 2, 12, 12, 64, 64, 3, 1, 1, True), dict(kind="WgradGeneric")),
    (("wgrad", 2, 8, 8, 64, 64, 3, 1, 1, False), dict(kind="WgradGeneric")),
    # 1x1 wgrad: stride 2 or pad 1 is not a GEMM; fp32 and P = 480 have no
    # slab route
    (("wgrad", 8, 8, 8, 256, 256, 1, 2, 0, True), dict(kind="WgradGeneric")),
    (("wgrad", 8, 8, 8, 256, 256, 1, 1, 1, True), dict(kind="WgradGeneric")),
    (("wgrad", 8, 8, 8, 256, 256, 1, 1, 0, False), SPLITK),
    (("wgrad", 30, 4, 4, 256, 256, 1, 1, 0, True), SPLITK),
    (("wgrad", 8, 8, 8, 256, 128, 1, 1, 0, True), SPLITK),
]


@pytest.mark.parametrize("shape,want", GATES)
def test_gates(shape, want):
    check(route(*shape), want, str(shape))


def test_bad_arguments_raise():
    with pytest.raises(RuntimeError):
        route("bgrad", 1, 8, 8, 32, 32, 3, 1, 1)
    with pytest.raises(RuntimeError):
        route("fwd", 1, 2, 2, 32, 32, 7, 1, 1)     # kernel > padded image
    with pytest.raises(RuntimeError):
        route("fwd", 0, 8, 8, 32, 32, 3, 1, 1)


def cdiv(a, b):
    return -(-a // b)


def covers(tiles, tile, extent):
    """tiles of `tile` cover `extent` with none to spare."""
    return (tiles - 1) * tile < extent <= tiles * tile


def test_random_routes_meet_launcher_preconditions():
    """Whatever the router picks, the kernel it names can run the shape, the
    grid covers the output exactly and the pixel slices tile [0, P)."""
    rng = random.Random(20250)
    extents = [1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 64, 128]
    chans = [3, 8, 32, 40, 64, 96, 128, 192, 256, 512]
    kinds = {}
    done = 0
    while done < 4000:
        op = rng.choice(["fwd", "dgrad", "wgrad"])
        N = rng.choice([1, 2, 3, 8, 30, 64, 256, 1024, 4096])
        H, W = rng.choice(extents), rng.choice(extents)
        Cin, Cout = rng.choice(chans), rng.choice(chans)
        KH = KW = rng.choice([1, 1, 2, 3, 3, 3, 7])
        if rng.random() < 0.1:
            KW = rng.choice([1, 3])
        s, p = rng.choice([1, 1, 1, 2, 2, 3]), rng.choice([0, 1, 1, 2, 3])
        bf16 = rng.random() < 0.75
        if rng.random() < 0.05:      # the 1x1 GEMM routes are rare otherwise
            KH = KW = s = 1
            p = 0
            Cin, Cout = rng.choice([256, 512]), rng.choice([128, 256, 512])
        if KH > H + 2 * p or KW > W + 2 * p or N * H * W > 1 << 26:
            continue
        done += 1
        r = OPS.conv_route(op, N, H, W, Cin, Cout, KH, KW, s, p, bf16=bf16)
        what = f"{op} {(N, H, W, Cin, Cout, KH, KW, s, p, bf16)} -> {r}"
        kind = r["kind"]
        kinds[kind] = kinds.get(kind, 0) + 1
        HO, WO = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
        assert r["out_hw"] == (HO, WO), what
        P = N * HO * WO
        M = N * H * W if op == "dgrad" else P
        cols, kc = (Cin, Cout) if op == "dgrad" else (Cout, Cin)
        gx, gy, gz = r["grid"]
        bm, bn = r["tile"]
        assert gx >= 1 and gy >= 1 and gz >= 1, what
        halo_ok = (op != "wgrad" and bf16 and (KH, KW, s, p) == (3, 3, 1, 1)
                   and 128 % W == 0 and H * W % 128 == 0 and kc % 32 == 0
                   and cols % 64 == 0)
        c8_ok = (op != "wgrad" and bf16 and (op == "fwd" or s == 1)
                 and cols % 256 == 0 and kc % 32 == 0
                 and KH * KW * kc % 64 == 0)
        c8_wanted = c8_ok and cdiv(M, 256) * (cols // 256) >= 256
        assert (kind == "Halo") == halo_ok, what
        assert (kind == "Conv8") == (c8_wanted and not halo_ok), what
        if kind == "Halo":
            R = 128 // W
            assert R <= H and H % R == 0, what       # tiles stay in one image
            assert 2 * (R + 2) * (W + 2) * 32 * 2 <= 160 * 1024, what
            assert (bm, bn) == (128, 64) and r["grid"] == \
                (M // 128, cols // 64, 1), what
        elif kind == "Conv8":
            assert KH * KW * kc >= 64, what          # at least one k-half
            assert (bm, bn) == (256, 256), what
            assert r["grid"] == (cols // 256, cdiv(M, 256), 1), what
            assert r["use_swz"] == 1
        elif kind in ("Generic", "DgradPhase"):
            assert op != "wgrad", what
            assert bm == 128 and bn == (64 if cols <= 64 else 128), what
            phase_ok = op == "dgrad" and s == 2 and Cout % 32 == 0
            assert (kind == "DgradPhase") == phase_ok, what
            if kind == "Generic":
                assert gz == 1 and covers(gx, bn, cols) and \
                    covers(gy, 128, M), what
                assert r["fast"] == (kc % 32 == 0), what
            else:
                rows = [N * cdiv(H - ph, 2) * cdiv(W - pw, 2)
                        for ph in (0, 1) for pw in (0, 1)]
                assert r["grid"] == (sum(cdiv(x, 128) for x in rows) *
                                     cdiv(cols, bn), 1, 1), what
        else:
            assert op == "wgrad", what
            assert r["splits"] == gz, what
            px_ok = OPS.wgrad_px_eligible(bf16, N, H, W, Cin, Cout, KH, KW,
                                          s, p)
            assert (kind == "WgradPx") == px_ok, what
            assert r["transpose_dy"] == (kind != "WgradPx"), what
            assert r["transpose_x"] == (kind == "Wgrad1x1Slab"), what
            gemm = (KH, KW, s, p) == (1, 1, 1, 0)
            assert kind.startswith("Wgrad1x1") == (gemm and not px_ok), what
            assert r["p_chunk"] % 32 == 0 and r["p_chunk"] >= 32, what
            if kind == "Wgrad1x1Slab":
                assert bf16 and Cin % 256 == 0 and Cout % 256 == 0, what
                assert gz > 1 and gz * r["p_chunk"] == P, what
                assert r["p_chunk"] >= 64, what
                assert r["grid"][:2] == (Cin // 256, Cout // 256), what
                assert r["gemm_kind"] == ("G9Slab" if r["p_chunk"] % 64 == 0
                                          else "G8Slab"), what
            else:
                assert covers(gz, r["p_chunk"], P), what
            if kind == "WgradPx":
                assert (bm, bn) == (64, 64) and \
                    (gx, gy) == (Cin // 64, Cout // 64), what
            elif kind == "WgradGeneric":
                assert bm == (64 if Cout <= 64 else 128) and bn == 128, what
                assert covers(gx, 128, KH * KW * Cin) and \
                    covers(gy, bm, Cout), what
            elif kind == "Wgrad1x1SplitK":
                assert covers(gx, bn, Cin) and covers(gy, bm, Cout), what
    # the sample reaches every kernel
    assert set(kinds) == {"Halo", "Conv8", "Generic", "DgradPhase", "WgradPx",
                          "WgradGeneric", "Wgrad1x1SplitK", "Wgrad1x1Slab"}, \
        kinds

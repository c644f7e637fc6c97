"""Phase map of the stride-2 conv dgrad (csrc/dgrad_phase_map.h), checked
without a GPU. ``dgrad_phase_map(N, H, W, KH, KW, stride, pad, BM)``
evaluates the very functions the kernel calls; everything here is compared
against the definition of the convolution, h = ho * s - p + kh, not against
the map."""

import itertools

import pytest

OPS = pytest.importorskip("baton_amd.ops._hip_ops")

N_IMG = 3
BM = 8                      # small tile: partial and multiple tiles per class
EXTENTS = [(4, 4), (5, 7), (6, 6), (1, 8), (32, 32)]
KERNELS = [(3, 2, 1), (1, 2, 0), (5, 2, 2), (3, 2, 0)]   # (K, stride, pad)
CASES = list(itertools.product(EXTENTS, KERNELS))


def out_extent(size, K, s, p):
    return (size + 2 * p - K) // s + 1


def phase_map(H, W, K, s, p, **kw):
    return OPS.dgrad_phase_map(N_IMG, H, W, K, K, s, p, BM, **kw)


@pytest.mark.parametrize("HW,Ksp", CASES)
def test_rows_are_a_bijection_with_input_pixels(HW, Ksp):
    (H, W), (K, s, p) = HW, Ksp
    m = phase_map(H, W, K, s, p)
    seen = []
    for c in m["classes"]:
        assert len(c["rows"]) == c["n_rows"] == N_IMG * c["Hc"] * c["Wc"]
        assert c["Hc"] == -(-(H - c["ph"]) // s) and c["Wc"] == -(-(W - c["pw"]) // s)
        for (n, h, w) in c["rows"]:
            assert (h % s, w % s) == (c["ph"], c["pw"])
            assert 0 <= n < N_IMG and 0 <= h < H and 0 <= w < W
        seen += c["rows"]
    assert len(seen) == N_IMG * H * W
    assert set(seen) == set(itertools.product(range(N_IMG), range(H), range(W)))
    assert sorted((c["ph"], c["pw"]) for c in m["classes"]) == \
        list(itertools.product(range(s), range(s)))


@pytest.mark.parametrize("HW,Ksp", CASES)
def test_contributions_match_the_definition(HW, Ksp):
    (H, W), (K, s, p) = HW, Ksp
    HO, WO = out_extent(H, K, s, p), out_extent(W, K, s, p)
    want = set()
    for n, ho, wo, kh, kw in itertools.product(
            range(N_IMG), range(HO), range(WO), range(K), range(K)):
        h, w = ho * s - p + kh, wo * s - p + kw
        if 0 <= h < H and 0 <= w < W:
            want.add((n, h, w, kh, kw, ho, wo))
    got = []
    for c in m_classes(H, W, K, s, p):
        taps = c["taps"]
        assert taps == sorted(taps), "taps not in ascending (kh, kw) order"
        for (n, h, w) in c["rows"]:
            a, b = (h - c["ph"]) // s, (w - c["pw"]) // s
            for (kh, kw, dh, dw) in taps:
                ho, wo = a + dh, b + dw       # the kernel's gather address
                if 0 <= ho < HO and 0 <= wo < WO:
                    got.append((n, h, w, kh, kw, ho, wo))
    assert len(got) == len(set(got)), "duplicate contribution"
    assert set(got) == want


def m_classes(H, W, K, s, p):
    return phase_map(H, W, K, s, p)["classes"]


@pytest.mark.parametrize("HW,Ksp", CASES)
def test_tiles_cover_rows_and_never_straddle_classes(HW, Ksp):
    (H, W), (K, s, p) = HW, Ksp
    m = phase_map(H, W, K, s, p)
    nxt = 0
    for c in m["classes"]:
        assert c["tile0"] == nxt, "tile ranges overlap or leave a gap"
        assert c["tiles"] == -(-c["n_rows"] // BM), "tiles do not cover the rows"
        nxt += c["tiles"]
    assert m["m_tiles"] == nxt


@pytest.mark.parametrize("HW,Ksp", CASES)
def test_class_order_and_empty_classes(HW, Ksp):
    (H, W), (K, s, p) = HW, Ksp
    classes = m_classes(H, W, K, s, p)
    assert len(classes) == s * s
    counts = [len(c["taps"]) for c in classes]
    assert counts == sorted(counts, reverse=True)
    assert sum(counts) == K * K, "every tap belongs to exactly one class"
    expect = {(3, 1): [4, 2, 2, 1], (1, 0): [1, 0, 0, 0],
              (5, 2): [9, 6, 6, 4], (3, 0): [4, 2, 2, 1]}[(K, p)]
    assert counts == expect
    if K == 1:
        # three classes have no taps but do have rows (written as zeros)
        empty = [c for c in classes if not c["taps"]]
        assert len(empty) == 3
        assert sum(c["n_rows"] for c in empty) == \
            N_IMG * H * W - N_IMG * -(-H // 2) * -(-W // 2)
        if H > 1 and W > 1:
            assert all(c["n_rows"] > 0 for c in empty)


@pytest.mark.parametrize("swz", [False, True])
@pytest.mark.parametrize("n_tiles", [1, 3])
@pytest.mark.parametrize("HW,Ksp", [((32, 32), (3, 2, 1)), ((5, 7), (3, 2, 1)),
                                    ((32, 32), (1, 2, 0)), ((1, 8), (3, 2, 1))])
def test_blocks_are_a_bijection_with_tiles(HW, Ksp, n_tiles, swz):
    """Block -> (class, M tile, N tile), with the per-class XCD remap (active
    from 64 blocks per class on: (32, 32) has 96 M tiles per class)."""
    (H, W), (K, s, p) = HW, Ksp
    m = phase_map(H, W, K, s, p, n_tiles=n_tiles, swz=swz)
    classes = m["classes"]
    want = {(ci, mt, nt) for ci, c in enumerate(classes)
            for mt in range(c["tiles"]) for nt in range(n_tiles)}
    blocks = m["blocks"]
    assert len(blocks) == len(want) == m["m_tiles"] * n_tiles
    assert set(blocks) == want
    # dispatch order walks the classes heaviest first
    assert [b[0] for b in blocks] == sorted(b[0] for b in blocks)
    if swz and H == 32 and K == 3:
        # every XCD (block id % 8) holds one contiguous run of each class
        start = 0
        for ci, c in enumerate(classes):
            nblk = c["tiles"] * n_tiles
            for lane in range(8):
                ids = sorted(mt * n_tiles + nt for (cc, mt, nt) in
                             blocks[start + lane:start + nblk:8])
                assert ids == list(range(ids[0], ids[0] + len(ids)))
            start += nblk

"""Index maps of the pixel-major 3x3 wgrad (csrc/wgrad_px_map.h), checked
without a GPU. ``wgrad_px_map(N, H, W, step)`` evaluates, for one k-step, the
very functions the kernel calls; everything here is compared against a
brute-force computation from (n, h, w) coordinates, not against the map.

Buffer layout under test: 160-byte rows; rows 0..31 the dy image, rows 32.. the
halo'd x window; chunk c = pass * 512 + thread lands at byte 16 c."""

import pytest

OPS = pytest.importorskip("baton_amd.ops._hip_ops")

N_IMG = 2
SHAPES = [(4, 4), (8, 8), (16, 16), (32, 32), (8, 16), (16, 4)]
ROWB = 160
CH_OFFS = (0, 32, 64, 96)          # 16-channel blocks within the 64-wide tile


def steps_of(H, W):
    return N_IMG * H * W // 32


def maps(H, W):
    return [OPS.wgrad_px_map(N_IMG, H, W, s) for s in range(steps_of(H, W))]


def coords(flat, H, W):
    return flat // (H * W), (flat // W) % H, flat % W


def lanes_of_kslot(k):
    """MFMA 16x16x32 operand: lane group g = k >> 3 holds k-values 8g..8g+7;
    transposed read r = (k >> 2) & 1 delivers 4 of them, element q = k & 3
    from the row whose address lanes 16g + 4q + p (p = 0..3) supply."""
    g, r, q = k >> 3, (k >> 2) & 1, k & 3
    return r, [(16 * g + 4 * q + p, p) for p in range(4)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_gather_map(H, W):
    for step, m in enumerate(maps(H, W)):
        assert m["row_bytes"] == ROWB
        kpix = m["kslot_pixel"]
        assert sorted(kpix) == list(range(32)), "k order is not a permutation"
        for k, px in enumerate(kpix):
            n, h, w = coords(32 * step + px, H, W)
            r, lanes = lanes_of_kslot(k)
            for lane, p in lanes:
                # A: the dy row holding this pixel
                a = m["a_addr"][r][lane]
                assert a % ROWB == 8 * p
                assert m["dy_rows"][a // ROWB] == px, (step, k, lane)
                # B: the window slot of every tap
                for t in range(9):
                    dh, dw = t // 3, t % 3
                    b = m["b_addr"][t][r][lane]
                    assert b % ROWB == 8 * p
                    slot = (b - m["window_base"]) // ROWB
                    assert 0 <= slot < m["slots"]
                    hh, ww = h + dh - 1, w + dw - 1
                    inside = 0 <= hh < H and 0 <= ww < W
                    want = (n, hh, ww) if inside else None
                    assert m["window"][slot] == want, (step, px, t, slot)


@pytest.mark.parametrize("H,W", SHAPES)
def test_read_alignment_and_bounds(H, W):
    for m in maps(H, W):
        reads = list(m["a_addr"]) + [m["b_addr"][t][r]
                                     for t in range(9) for r in range(2)]
        for addrs in reads:
            assert len(addrs) == 64
            for a in addrs:
                for off in CH_OFFS:
                    assert (a + off) % 8 == 0
                    assert 0 <= a + off and a + off + 8 <= m["buffer_bytes"]
                    # inside the 128 data bytes of its row, never the pad
                    assert (a + off) % ROWB + 8 <= 128


def conflict_degree(addrs):
    """Guide rule for ds_read_b64_tr_b16: bank = (addr / 4) % 64, counted per
    32-lane half, each lane touching 2 consecutive banks."""
    worst = 0
    for half in (addrs[:32], addrs[32:]):
        hits = {}
        for a in half:
            for b in ((a // 4) % 64, (a // 4 + 1) % 64):
                hits[b] = hits.get(b, 0) + 1
        worst = max(worst, max(hits.values()))
    return worst


@pytest.mark.parametrize("H,W", SHAPES)
def test_bank_conflicts(H, W):
    for m in maps(H, W):
        claimed = m["claimed_conflict_degree"]
        assert claimed == 1              # what the kernel comment states
        for r in range(2):
            for off in CH_OFFS:
                a = [x + off for x in m["a_addr"][r]]
                assert conflict_degree(a) == claimed, ("A", r, off)
                for t in range(9):
                    b = [x + off for x in m["b_addr"][t][r]]
                    assert conflict_degree(b) == claimed, ("B", t, r, off)


@pytest.mark.parametrize("H,W", SHAPES)
def test_staging_map(H, W):
    for step, m in enumerate(maps(H, W)):
        assert len(m["stage"]) == m["passes"] * m["threads"]
        assert m["buffer_bytes"] == 16 * len(m["stage"])
        writers = {}
        for pas, tid, dst, kind, px, sub in m["stage"]:
            assert dst == 16 * (pas * m["threads"] + tid)   # lane-linear
            assert dst not in writers
            writers[dst] = (kind, px, sub)
        rows = 32 + m["slots"]
        assert rows * ROWB <= m["buffer_bytes"]
        for row in range(rows):
            for sub in range(8):
                # every data chunk has exactly one writer (dict + the
                # uniqueness assert above), carrying the right channel run
                kind, px, s = writers[row * ROWB + 16 * sub]
                if row < 32:
                    assert kind == 1 and s == sub
                    assert px == 32 * step + m["dy_rows"][row]
                else:
                    want = m["window"][row - 32]
                    if want is None:
                        assert kind == 0
                    else:
                        assert kind == 2 and s == sub
                        assert coords(px, H, W) == want
            for sub in (8, 9):          # pad chunks read the zero page
                assert writers[row * ROWB + 16 * sub][0] == 0


def test_gate():
    el = OPS.wgrad_px_eligible
    for H, W in SHAPES:
        assert el(True, 2, H, W, 64, 128, 3, 3, 1, 1)
    assert not el(False, 2, 8, 8, 64, 64, 3, 3, 1, 1)      # fp32
    assert not el(True, 2, 12, 12, 64, 64, 3, 3, 1, 1)     # W does not divide 32
    assert not el(True, 2, 6, 8, 64, 64, 3, 3, 1, 1)       # H % rows-per-step
    assert not el(True, 1, 4, 4, 64, 64, 3, 3, 1, 1)       # half a k-step
    assert not el(True, 2, 8, 8, 96, 64, 3, 3, 1, 1)       # Cin % 64
    assert not el(True, 2, 8, 8, 64, 64, 3, 3, 2, 1)       # stride 2
    assert not el(True, 2, 8, 8, 64, 64, 1, 1, 1, 0)       # 1x1

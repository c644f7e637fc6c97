// Phase decomposition of the stride-2 conv dgrad (conv.hip,
// conv_dgrad_phase_kernel): plain integer functions, usable from host and
// device, so the whole map can be checked on a machine with no GPU
// (dgrad_phase_map() in bindings.cpp, tests/test_dgrad_phase_map.py). The
// kernel calls these same functions; it keeps no copy.
//
// dx[n, h, w, :] = sum over (kh, kw) with h + pad - kh = s * ho and
// w + pad - kw = s * wo of dy[n, ho, wo, :] @ w[:, kh, kw, :]. For stride s
// an input pixel of class (ph, pw) = (h % s, w % s) is reached only by taps
// with (ph + pad - kh) % s == 0 and (pw + pad - kw) % s == 0: a 3x3 s2 p1
// conv gives the four classes 4, 2, 2 and 1 taps, a 1x1 s2 p0 conv 1, 0, 0
// and 0. Inside a class h = s * a + ph, w = s * b + pw and a tap reads
// dy[n, a + dh, b + dw] with dh = (ph + pad - kh) / s (exact, may be
// negative), dw likewise: a stride-1 walk over dy with a short constant tap
// list. Every tap belongs to exactly one class, so the classes' lists
// partition the KH * KW taps.
//
// Rows of the GEMM are laid out class by class, each class in (n, a, b)
// order and tiled by BM on its own, so no M tile straddles two classes and
// a block's K loop is its class's taps x Cout. Classes are ordered by tap
// count, heaviest first, so the blocks dispatched last are the short ones.
// A class without taps still has rows (they are written as zeros).
//
// The map is small (360 bytes) and travels by value in the kernel's
// argument struct: no device table, no copy, nothing to go stale under
// graph replay.
#pragma once

#if defined(__HIPCC__)
#define DGPH_HD __host__ __device__ inline
#else
#define DGPH_HD inline
#endif

namespace dgph {

constexpr int STRIDE = 2;
constexpr int NCLS = STRIDE * STRIDE;
constexpr int MAX_TAPS = 49;   // KH * KW of the largest kernel taken (7x7)

struct Tap {
  signed char kh, kw;   // weight tap
  signed char dh, dw;   // ho = a + dh, wo = b + dw
};

struct Class {
  int ph, pw;           // h % STRIDE, w % STRIDE
  int Hc, Wc;           // class extents: a in [0, Hc), b in [0, Wc)
  int rows;             // N * Hc * Wc
  int tile0, tiles;     // first M tile, ceil(rows / BM)
  int tap0, ntaps;      // this class's run in Map::taps, ascending (kh, kw)
};

struct Map {
  int N, H, W, BM;
  int m_tiles;          // sum of the classes' tiles
  Class cls[NCLS];      // heaviest first
  Tap taps[MAX_TAPS];
};

// The launcher's gate (cbk = k-step width of the kernel). Everything else
// keeps the generic dgrad kernel.
DGPH_HD bool eligible(int N, int H, int W, int Cout, int KH, int KW,
                      int stride, int pad, int cbk) {
  if (stride != STRIDE || Cout % cbk != 0) return false;
  if (KH < 1 || KW < 1 || KH * KW > MAX_TAPS || pad < 0 || pad > 63)
    return false;
  // rows and flat pixels are ints, with room for one tile of overshoot
  return (long long)N * H * W < (1LL << 31) - 4096;
}

// taps of one parity along one axis: k with (p + pad - k) % STRIDE == 0
DGPH_HD int axis_taps(int p, int pad, int K) {
  const int k0 = (p + pad) % STRIDE;
  return K > k0 ? (K - k0 + STRIDE - 1) / STRIDE : 0;
}

DGPH_HD Map make_map(int N, int H, int W, int KH, int KW, int pad, int BM) {
  Map m{};
  m.N = N; m.H = H; m.W = W; m.BM = BM;
  int order[NCLS], count[NCLS];
  for (int c = 0; c < NCLS; ++c) {
    order[c] = c;
    count[c] = axis_taps(c / STRIDE, pad, KH) * axis_taps(c % STRIDE, pad, KW);
  }
  // stable insertion sort, tap count descending
  for (int i = 1; i < NCLS; ++i)
    for (int j = i; j > 0 && count[order[j]] > count[order[j - 1]]; --j) {
      const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t;
    }
  int tile = 0, tap = 0;
  for (int i = 0; i < NCLS; ++i) {
    Class& c = m.cls[i];
    c.ph = order[i] / STRIDE;
    c.pw = order[i] % STRIDE;
    c.Hc = H > c.ph ? (H - c.ph + STRIDE - 1) / STRIDE : 0;
    c.Wc = W > c.pw ? (W - c.pw + STRIDE - 1) / STRIDE : 0;
    c.rows = N * c.Hc * c.Wc;
    c.tile0 = tile;
    c.tiles = (c.rows + BM - 1) / BM;
    tile += c.tiles;
    c.tap0 = tap;
    for (int kh = 0; kh < KH; ++kh) {
      const int hn = c.ph + pad - kh;
      if (hn % STRIDE != 0) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int wn = c.pw + pad - kw;
        if (wn % STRIDE != 0) continue;
        Tap& t = m.taps[tap++];
        t.kh = (signed char)kh; t.kw = (signed char)kw;
        t.dh = (signed char)(hn / STRIDE); t.dw = (signed char)(wn / STRIDE);
      }
    }
    c.ntaps = tap - c.tap0;
  }
  m.m_tiles = tile;
  return m;
}

// class row r (0 .. rows-1) -> (n, a, b)
struct RowPos { int n, a, b; };
DGPH_HD RowPos row_pos(const Class& c, int r) {
  RowPos p;
  p.b = r % c.Wc;
  const int t = r / c.Wc;
  p.a = t % c.Hc;
  p.n = t / c.Hc;
  return p;
}

// class row -> flat input pixel (n * H + h) * W + w
DGPH_HD int row_pixel(const Map& m, const Class& c, int r) {
  const RowPos p = row_pos(c, r);
  return (p.n * m.H + STRIDE * p.a + c.ph) * m.W + STRIDE * p.b + c.pw;
}

// Block -> tile. Blocks are numbered class by class in dispatch order (so
// the heaviest class starts first), n tile fastest. The dispatcher places
// block b on XCD b % 8; with swz, each class's blocks are renumbered by the
// XCD remap of common.h on their own, so every XCD gets one contiguous run
// of EVERY class. (One remap over the whole grid would hand the 4-tap
// class to the first XCDs and the 1-tap class to the last.) A class's first
// block is in general not on XCD 0: lanes of the remap are the class-local
// b % 8, a fixed rotation of the XCD number, which serves as well.
struct Tile { int cls, m_tile, n_tile; };   // m_tile counts within the class
DGPH_HD Tile block_tile(const Map& m, int bid, int n_tiles, int swz) {
  int c = 0;
  for (int i = 1; i < NCLS; ++i)
    if (bid >= m.cls[i].tile0 * n_tiles) c = i;
  int local = bid - m.cls[c].tile0 * n_tiles;
  const int nwg = m.cls[c].tiles * n_tiles;
  if (swz && nwg >= 64) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = local & 7, idx = local >> 3;
    local = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  Tile t;
  t.cls = c;
  t.n_tile = local % n_tiles;
  t.m_tile = local / n_tiles;
  return t;
}

}  // namespace dgph

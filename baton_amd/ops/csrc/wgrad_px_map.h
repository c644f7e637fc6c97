// Index maps of the pixel-major 3x3 stride-1 wgrad (conv_wgrad_px.hip):
// plain integer functions, usable from host and device, so every map the
// kernel relies on can be checked on a machine with no GPU
// (wgrad_px_map() in bindings.cpp, tests/test_wgrad_px_map.py). The kernel
// calls these same functions; it keeps no copy.
//
// One k-step is 32 consecutive flat pixels (PXK), i.e. R = 32 / W whole
// image rows. An LDS buffer is one lane-linear array of 16-B chunks holding
// ROWB-byte rows of 64 channels (128 B data + 32 B pad):
//   rows 0 .. 31        dy image: row rho holds step pixel lin_pixel(W, rho)
//   rows 32 .. 32+slots x window: one halo'd copy of the step's pixels that
//                       serves all 9 taps
// Window slot of image position (window row j, column c in -1 .. W):
//   slot = j * pitch + c + 1
// pitch is W + 1 (the right border of one row IS the left border of the
// next, both zero) except W == 4, which keeps both borders (pitch 6) for
// the bank placement below. Window row of step row i is 1 + i, plus one
// shared zero row per image boundary inside the step (H < R: the step
// covers R / H whole images), so a tap (dh, dw) is the constant slot offset
// dh * pitch + dw from the slot of tap (0, 0).
//
// Bank placement (ds_read_b64_tr_b16: bank = (addr / 4) % 64 per 32-lane
// half, 2 banks per lane). A 16-lane group reads 4 rows x 32 B; a half
// reads 8 rows. With 160-B rows, row s starts at bank 40 s % 64 = 8 (5 s %
// 8), so 8 rows whose slots are distinct mod 8 tile the 64 banks exactly:
// conflict-free (degree 1). The k order guarantees it: k-slot 8g + 4r + e
// (lane group g, read r, element e) holds position lin = 16r + 4g + e, so
// a half's two groups read positions 16r + 8h + [0, 8) - 8 consecutive dy
// rows, and 8 consecutive window slots for W >= 8. For W == 4 positions
// map to pixels so that a half takes step rows {i, i + 2}: slots s .. s+3
// and s + 12 .. s + 15 (pitch 6), again distinct mod 8. K is summed, so
// any assignment works as long as A (dy) and B (x) share it.
#pragma once

#if defined(__HIPCC__)
#define WGPX_HD __host__ __device__ inline
#else
#define WGPX_HD inline
#endif

namespace wgpx {

constexpr int PXK = 32;        // pixels per k-step
constexpr int TILE = 64;       // co tile == ci tile
constexpr int THREADS = 512;
constexpr int ROWB = 160;      // LDS row pitch in bytes
constexpr int CPR = ROWB / 16; // 16-B chunks per row (8 data + 2 pad)
constexpr int NBUF = 3;        // LDS buffers (two k-steps of glds in flight)

constexpr int pitch_of(int W) { return W == 4 ? 6 : W + 1; }
// staging passes (chunks / THREADS, rounded up) at the gate's H >= 4
constexpr int passes_of(int W) { return W == 32 ? 3 : 2; }

struct Geom {
  int H, W;
  int R;       // image rows per k-step
  int pitch;   // window slots per window row
  int wrows;   // window rows
  int slots;   // window slots (wrows * pitch + 1)
  int chunks;  // 16-B chunks that hold data or pad: (32 + slots) * CPR
};

// The launcher's gate. Everything else goes to the generic wgrad kernel.
WGPX_HD bool eligible(bool is_bf16, int N, int H, int W, int Cin, int Cout,
                      int KH, int KW, int stride, int pad) {
  if (!is_bf16 || KH != 3 || KW != 3 || stride != 1 || pad != 1) return false;
  if (Cin % TILE || Cout % TILE) return false;
  if (W != 4 && W != 8 && W != 16 && W != 32) return false;
  const int R = PXK / W;
  if (H < 4) return false;                       // keeps passes_of(W) exact
  if (H >= R ? (H % R) != 0 : (R % H) != 0) return false;
  if (((long long)N * H * W) % PXK) return false;  // whole k-steps only
  return true;
}

WGPX_HD Geom make_geom(int H, int W) {
  Geom g;
  g.H = H; g.W = W;
  g.R = PXK / W;
  g.pitch = pitch_of(W);
  g.wrows = g.R + 2 + (H < g.R ? g.R / H - 1 : 0);
  g.slots = g.wrows * g.pitch + 1;
  g.chunks = (PXK + g.slots) * CPR;
  return g;
}

// position in the k order (== dy LDS row) -> pixel of the step
WGPX_HD int lin_pixel(int W, int lin) {
  if (W != 4) return lin;
  const int m = lin >> 3, e = lin & 7;
  const int row = (m & 1) + 4 * (m >> 1) + 2 * (e >> 2);
  return row * 4 + (e & 3);
}

// MFMA k index (lane group g = k >> 3, read r = (k >> 2) & 1, element
// e = k & 3) -> position in the k order
WGPX_HD int kslot_lin(int k) {
  return 16 * ((k >> 2) & 1) + 4 * (k >> 3) + (k & 3);
}

// step row i (0 .. R-1) -> window row
WGPX_HD int win_row(const Geom& g, int i) {
  return 1 + i + (g.H < g.R ? i / g.H : 0);
}

// step pixel -> window slot of tap (0, 0), i.e. of image position (h-1, w-1)
WGPX_HD int pix_slot0(const Geom& g, int px) {
  return (win_row(g, px / g.W) - 1) * g.pitch + (px % g.W);
}

WGPX_HD int tap_off(const Geom& g, int dh, int dw) { return dh * g.pitch + dw; }
constexpr int tap_bytes(int W, int dh, int dw) {
  return (dh * pitch_of(W) + dw) * ROWB;
}

// Source of one staged 16-B chunk. The destination is lane-linear: chunk c
// = pass * THREADS + thread goes to byte 16 c of the buffer.
struct ChunkSrc {
  int kind;       // 0: zero page, 1: dy, 2: x
  int rel;        // pixel relative to the step's first flat pixel
  int sub;        // 8-channel run within the 64-channel tile
  // x only: the chunk is real data iff 0 <= h0 + hrel < H, where h0 is the
  // image row of the step's first pixel; else it takes the zero page
  int hrel;
};

WGPX_HD ChunkSrc chunk_src(const Geom& g, int c) {
  ChunkSrc s{0, 0, 0, 0};
  const int row = c / CPR, sub = c % CPR;
  if (sub >= 8 || row >= PXK + g.slots) return s;     // pad / past the end
  s.sub = sub;
  if (row < PXK) {
    s.kind = 1;
    s.rel = lin_pixel(g.W, row);
    return s;
  }
  const int slot = row - PXK;
  const int j = slot / g.pitch, w = slot % g.pitch - 1;
  if (j >= g.wrows || w < 0 || w >= g.W) return s;    // border column
  int img = 0, hrel = j - 1;
  if (g.H < g.R) {                                    // whole images per step
    img = j / (g.H + 1);
    hrel = j % (g.H + 1) - 1;
    if (hrel < 0) return s;                           // shared zero row
  }
  s.kind = 2;
  s.rel = (img * g.H + hrel) * g.W + w;
  s.hrel = hrel;
  return s;
}

WGPX_HD bool x_row_valid(const Geom& g, int h0, int hrel) {
  return (unsigned)(h0 + hrel) < (unsigned)g.H;
}

// Per-lane byte address (relative to the buffer) of transposed read r (0/1)
// of the A operand, co block 0: lane 16g + 4q + p supplies row q of its
// group's block, columns 4p .. 4p+3. A co block further on adds 32 B.
WGPX_HD int a_read_addr(int lane, int r) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return (16 * r + 4 * g + q) * ROWB + 8 * p;
}

// Same for the B operand at tap (0, 0), ci block 0. A tap adds
// tap_off() * ROWB, a ci block 32 B.
WGPX_HD int b_read_addr(const Geom& g, int lane, int r) {
  const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int px = lin_pixel(g.W, 16 * r + 4 * gq + q);
  return (PXK + pix_slot0(g, px)) * ROWB + 8 * p;
}

// K split: k-steps per grid.z slice. The fp32 atomic volume is splits x
// tile bytes, so aim at ~2 blocks per CU (512 blocks) and no finer.
WGPX_HD int steps_per_split(long long steps, int tiles) {
  int target = 512 / tiles;
  if (target < 1) target = 1;
  long long splits = steps < target ? steps : target;
  return (int)((steps + splits - 1) / splits);
}

}  // namespace wgpx

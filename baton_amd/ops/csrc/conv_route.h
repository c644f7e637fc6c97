// Host-side conv router: which kernel, tile, grid and pixel split a
// convolution gets. Pure (no HIP, no torch, no environment), like
// gemm_plan.h, so every routing decision can be checked without a GPU;
// bindings.cpp executes the route and the launchers in conv.hip, conv8.hip,
// conv_halo.hip and conv_wgrad_px.hip launch exactly what it names. A
// launcher handed a route or a shape its kernel cannot run returns false
// and launches nothing; bindings.cpp turns that into a hard error.
//
// Layouts: x [N,H,W,Cin], w [Cout,KH,KW,Cin], y / dy [N,HO,WO,Cout], NHWC.
#pragma once

#include "dgrad_phase_map.h"
#include "gemm_plan.h"
#include "wgrad_px_map.h"

enum class ConvOp { Fwd, Dgrad, Wgrad };
constexpr const char* kConvOpName[] = {"fwd", "dgrad", "wgrad"};

enum class ConvKind {
  Halo,            // conv_halo.hip, shared-halo 3x3 s1 p1 fwd / dgrad
  Conv8,           // conv8.hip, 256x256 8-wave fwd / stride-1 dgrad
  Generic,         // conv.hip, conv_fwd_kernel / conv_dgrad_kernel
  DgradPhase,      // conv.hip, conv_dgrad_phase_kernel (stride 2)
  WgradPx,         // conv_wgrad_px.hip, pixel-major 3x3 s1 p1 wgrad
  WgradGeneric,    // conv.hip, conv_wgrad_kernel on the transposed dy
  Wgrad1x1SplitK,  // gemm.hip, NN split-K GEMM dw = dy_t @ x
  Wgrad1x1Slab,    // gemm8.hip, NT slab GEMM dw = dy_t @ x_t^T
};
constexpr const char* kConvKindName[] = {
    "Halo",    "Conv8",        "Generic",        "DgradPhase",
    "WgradPx", "WgradGeneric", "Wgrad1x1SplitK", "Wgrad1x1Slab"};

struct ConvProblem {
  ConvOp op;
  bool bf16;   // compute dtype (else fp32)
  int N, H, W, Cin, Cout, KH, KW, stride, pad;
};

struct ConvRoute {
  ConvKind kind;
  int HO, WO;
  int bm, bn;          // output tile: rows x columns of the implicit GEMM
  bool fast;           // Generic only: the stagers' channels % 32 == 0 path
  int grid_x, grid_y, grid_z;
  int splits;          // wgrad: slices of the pixel contraction; else 1
  long long p_chunk;   // wgrad: pixels per slice; else 0
  int use_swz;         // XCD block remap requested (kernels apply it from 64
                       // blocks up)
  bool transpose_dy;   // wgrad: dy re-laid-out to [Cout][P] first
  bool transpose_x;    // Wgrad1x1Slab: x re-laid-out to [Cin][P] first
  GemmPlan gemm;       // the 1x1 wgrad routes: the GEMM plan to execute
};

constexpr int kConvBK = 32;         // k-step of every conv kernel
constexpr int kConvBM = 128;        // generic kernels: pixel rows per tile
constexpr int kHaloPx = 128;        // halo kernel: pixel tile
constexpr int kHaloNT = 64;         // halo kernel: filter tile
constexpr long long kHaloMaxLds = 160 * 1024;
constexpr int kConv8Tile = 256;     // conv8: 256x256 tile
// one 8-wave block per CU: below 256 blocks the 2-phase kernels fill better
constexpr long long kConv8MinBlocks = 256;
// XCD swizzle only when the activations exceed the 256 MiB L3 (see
// kSwizzleBytes in gemm_plan.h)
constexpr long long kConvSwizzleBytes = 200LL << 20;
// generic wgrad: split the pixels to fill ~2 blocks per CU
constexpr int kWgradTargetBlocks = 512;

inline int conv_out(int in, int k, int stride, int pad) {
  return (in + 2 * pad - k) / stride + 1;
}

// Rows / columns / contraction length of the implicit GEMM of fwd and dgrad.
inline long long conv_rows(const ConvProblem& p) {
  if (p.op == ConvOp::Dgrad) return (long long)p.N * p.H * p.W;
  return (long long)p.N * conv_out(p.H, p.KH, p.stride, p.pad) *
         conv_out(p.W, p.KW, p.stride, p.pad);
}
inline int conv_cols(const ConvProblem& p) {   // output channels of the op
  return p.op == ConvOp::Dgrad ? p.Cin : p.Cout;
}
inline int conv_kchan(const ConvProblem& p) {  // contracted channels
  return p.op == ConvOp::Dgrad ? p.Cout : p.Cin;
}

// ---- what each kernel can run (the launchers refuse anything else) ---------

// conv_halo.hip: 3x3 stride 1 pad 1 bf16, a 128-pixel tile is R = 128 / W
// whole rows of one image, 32-channel k-steps, 64-filter tiles, and the two
// halo images fit the LDS.
inline bool conv_halo_fits(const ConvProblem& p) {
  if (p.op == ConvOp::Wgrad || !p.bf16) return false;
  if (p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1) return false;
  if (p.W < 1 || kHaloPx % p.W != 0) return false;
  if ((long long)p.H * p.W % kHaloPx != 0) return false;
  if (conv_kchan(p) % kConvBK != 0 || conv_cols(p) % kHaloNT != 0) return false;
  const int R = kHaloPx / p.W;
  if (R > p.H) return false;
  return 2LL * (R + 2) * (p.W + 2) * kConvBK * 2 <= kHaloMaxLds;
}

// conv8.hip: bf16, dgrad stride 1 only, full 256-column tiles, 32-channel
// k-halves within one tap, at least one k-half. Rows may be ragged: the A
// stager points rows past M at the zero page and the epilogue skips them.
inline bool conv8_fits(const ConvProblem& p) {
  if (p.op == ConvOp::Wgrad || !p.bf16) return false;
  if (p.op == ConvOp::Dgrad && p.stride != 1) return false;
  if (conv_cols(p) % kConv8Tile != 0 || conv_kchan(p) % kConvBK != 0)
    return false;
  return p.KH * p.KW * conv_kchan(p) % 64 == 0;
}

// conv_dgrad_phase_kernel
inline bool conv_dgrad_phase_fits(const ConvProblem& p) {
  return p.op == ConvOp::Dgrad &&
         dgph::eligible(p.N, p.H, p.W, p.Cout, p.KH, p.KW, p.stride, p.pad,
                        kConvBK);
}

// conv_wgrad_px.hip
inline bool conv_wgrad_px_fits(const ConvProblem& p) {
  return p.op == ConvOp::Wgrad &&
         wgpx::eligible(p.bf16, p.N, p.H, p.W, p.Cin, p.Cout, p.KH, p.KW,
                        p.stride, p.pad);
}

// ---- the route -------------------------------------------------------------

// Generic fwd / dgrad tile: 128 pixels x 64 columns when the op's output
// channels fit one narrow tile (stem / layer1), else 128 x 128.
inline void conv_set_generic(ConvRoute& rt, const ConvProblem& p) {
  rt.bm = kConvBM;
  rt.bn = conv_cols(p) <= 64 ? 64 : 128;
  const long long act = (long long)p.N * p.H * p.W * p.Cin +
                        (long long)p.N * rt.HO * rt.WO * p.Cout;
  rt.use_swz = act * 2 > kConvSwizzleBytes ? 1 : 0;
}

inline ConvRoute conv_route(const ConvProblem& p) {
  ConvRoute rt{};
  rt.HO = conv_out(p.H, p.KH, p.stride, p.pad);
  rt.WO = conv_out(p.W, p.KW, p.stride, p.pad);
  rt.splits = 1;
  rt.grid_z = 1;

  if (p.op != ConvOp::Wgrad) {
    const long long M = conv_rows(p);
    const int cols = conv_cols(p);
    // 3x3 stride-1 small-channel layers: one halo image serves all 9 taps
    if (conv_halo_fits(p)) {
      rt.kind = ConvKind::Halo;
      rt.bm = kHaloPx;
      rt.bn = kHaloNT;
      rt.grid_x = (int)(M / kHaloPx);
      rt.grid_y = cols / kHaloNT;
      return rt;
    }
    // 256-column layers whose pixel grid covers the chip
    const long long mt = (M + kConv8Tile - 1) / kConv8Tile;
    if (conv8_fits(p) && mt * (cols / kConv8Tile) >= kConv8MinBlocks) {
      rt.kind = ConvKind::Conv8;
      rt.bm = rt.bn = kConv8Tile;
      rt.grid_x = cols / kConv8Tile;
      rt.grid_y = (int)mt;
      rt.use_swz = 1;
      return rt;
    }
    conv_set_generic(rt, p);
    const int n_tiles = (cols + rt.bn - 1) / rt.bn;
    // stride-2 dgrad: only the live taps of each parity class
    if (conv_dgrad_phase_fits(p)) {
      rt.kind = ConvKind::DgradPhase;
      const dgph::Map mp =
          dgph::make_map(p.N, p.H, p.W, p.KH, p.KW, p.pad, kConvBM);
      rt.grid_x = mp.m_tiles * n_tiles;
      rt.grid_y = 1;
      return rt;
    }
    rt.kind = ConvKind::Generic;
    rt.fast = conv_kchan(p) % kConvBK == 0;
    rt.grid_x = n_tiles;
    rt.grid_y = (int)((M + kConvBM - 1) / kConvBM);
    return rt;
  }

  // wgrad: dw[Cout][KH*KW*Cin] = sum over the P = N*HO*WO pixels
  const long long P = (long long)p.N * rt.HO * rt.WO;
  // 3x3 stride-1: the pixel-major kernel reads dy as it is
  if (conv_wgrad_px_fits(p)) {
    rt.kind = ConvKind::WgradPx;
    rt.bm = rt.bn = wgpx::TILE;
    rt.grid_x = p.Cin / wgpx::TILE;
    rt.grid_y = p.Cout / wgpx::TILE;
    const long long steps = P / wgpx::PXK;
    const int sps = wgpx::steps_per_split(steps, rt.grid_x * rt.grid_y);
    rt.splits = rt.grid_z = (int)((steps + sps - 1) / sps);
    rt.p_chunk = (long long)sps * wgpx::PXK;
    return rt;
  }
  // every other route wants dy transposed once ([P,Cout] -> [Cout,P]) so the
  // wgrad A operand is k (= pixel) contiguous
  rt.transpose_dy = true;
  if (p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0) {
    // 1x1 stride-1 wgrad IS a dense GEMM: dw[Cout,Cin] = dy_t[Cout,P] @
    // x[P,Cin], NN, K = pixels - the split-K GEMM runs it at GEMM speed (the
    // conv-path x gather measured ~68 TF on these shapes, the NN split-K
    // ~250 TF). When Cout / Cin are 256-divisible, x is transposed too and
    // the 8-wave slab kernel takes it (the rn50 bottleneck 1x1 wgrads were
    // 12% of the step on the atomic path).
    int splits = 1;
    if (p.bf16 && p.Cout % kTile8 == 0 && p.Cin % kTile8 == 0)
      splits = slab_splits((long long)(p.Cout / kTile8) * (p.Cin / kTile8),
                           (int)P);
    if (splits > 1) {
      rt.kind = ConvKind::Wgrad1x1Slab;
      rt.transpose_x = true;
      rt.gemm = plan_slab(p.Cout, p.Cin, (int)P, splits);
    } else {
      rt.kind = ConvKind::Wgrad1x1SplitK;
      rt.gemm = plan_splitk(1, p.Cout, p.Cin, (int)P);
    }
    rt.bm = rt.gemm.bm;
    rt.bn = rt.gemm.bn;
    rt.grid_x = rt.gemm.grid_x;
    rt.grid_y = rt.gemm.grid_y;
    rt.grid_z = rt.gemm.grid_z;
    rt.splits = rt.gemm.splits;
    rt.p_chunk = rt.gemm.k_chunk;
    rt.use_swz = rt.gemm.use_swz;
    return rt;
  }
  // generic wgrad: 64-row tiles for 64-filter layers; pixel slices of whole
  // k-steps over grid.z, fp32 atomics
  rt.kind = ConvKind::WgradGeneric;
  rt.bm = p.Cout <= 64 ? 64 : 128;
  rt.bn = 128;
  rt.grid_x = (p.KH * p.KW * p.Cin + 127) / 128;
  rt.grid_y = (p.Cout + rt.bm - 1) / rt.bm;
  int target = kWgradTargetBlocks / (rt.grid_x * rt.grid_y);
  if (target < 1) target = 1;
  const long long max_splits = (P + kConvBK - 1) / kConvBK;
  const int want = (int)(max_splits < target ? max_splits : target);
  rt.p_chunk = ((P + want - 1) / want + kConvBK - 1) / kConvBK * kConvBK;
  rt.splits = rt.grid_z = (int)((P + rt.p_chunk - 1) / rt.p_chunk);
  return rt;
}

// A route the launchers accept for `p`: the kind's kernel can run the shape
// and the grid covers the output exactly.
inline bool conv_grid_fits(const ConvRoute& rt, const ConvProblem& p, int bm,
                           int bn) {
  return rt.bm == bm && rt.bn == bn && rt.grid_z == 1 &&
         rt.grid_x == (conv_cols(p) + bn - 1) / bn &&
         rt.grid_y == (conv_rows(p) + bm - 1) / bm;
}

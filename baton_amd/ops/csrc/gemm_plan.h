// Host-side GEMM planner: which kernel, tile, grid and K split a problem
// gets. Pure (no HIP, no torch, no environment), so every routing decision
// can be checked without a GPU; bindings.cpp executes the plan and the
// launchers in gemm.hip / gemm8.hip launch exactly what it names.
#pragma once

enum class GemmKind {
  TwoPhase,        // gemm.hip, dense
  TwoPhaseSplitK,  // gemm.hip, K slices over grid.z, fp32 atomics
  G9,              // gemm8.hip, 256x256 8-wave fine-phase NT kernel, dense
  G9Slab,          // gemm8.hip, g9 split-K into fp32 slabs + reduce
  G8Slab,          // gemm8.hip, the slab kernel for k_chunk % 64 == 32
};
constexpr const char* kGemmKindName[] = {"TwoPhase", "TwoPhaseSplitK", "G9",
                                         "G9Slab", "G8Slab"};

struct GemmProblem {
  bool bf16;            // compute dtype (else fp32)
  bool out_f32;
  int layout;           // 0 = NT, 1 = NN, 2 = TN
  int M, N, K;
  bool has_bias, relu;
  double alpha, beta;
  bool direct;          // caller forbids the transpose-to-NT re-layouts
  int nbatch;
  bool strided;         // GemmStrides in use (attention views)
};

struct GemmPlan {
  bool transpose_a, transpose_b;   // re-lay the operand out to NT first
  int layout;                      // effective layout after the transposes
  GemmKind kind;
  int bm, bn;                      // output tile
  int grid_x, grid_y, grid_z;
  int splits, k_chunk;             // split routes; 1 / K otherwise
  int use_swz;                     // XCD block remap
  // Rows this plan covers. Less than M only for ragged-M G9: the remaining
  // M - m_main rows get the plan of gemm_remainder().
  int m_main;
};

constexpr int kGemmBK = 32;        // K-step of the 2-phase kernel
constexpr int kTile8 = 256;        // 8-wave kernels: 256x256 tile
// split-K when the tile grid underfills the chip and K is long
constexpr long long kSplitKMaxTiles = 256;
constexpr int kSplitKMinK = 1024;
// slab route: at most this many 8-wave blocks over all K slices, and
// slices no shorter than kSlabMinChunk
constexpr long long kSlabMaxBlocks = 384;
constexpr int kSlabMinChunk = 256;
// one 8-wave block per CU: the grid must roughly cover the 256 CUs or
// the higher-occupancy 2-phase kernel wins (measured: 554 vs 871 TF at
// 128 blocks; at 192 blocks the 8-phase already wins — BERT fwd N=768
// shapes, r2 A/B +1%)
constexpr long long kG9MinBlocks = 160;
// NN dgrad routing: below this many B bytes the native NN staging beats a
// transpose-to-NT pass (measured on BERT-base dgrad shapes)
constexpr long long kNNTransposeBytes = 1 << 20;
// XCD swizzle only when the operands exceed the 256 MiB L3 (T1: costs a
// few % when L3-resident, pays ~10% when HBM-bound)
constexpr long long kSwizzleBytes = 200LL << 20;
// Dense tile geometry: prefer 128x128; when that grid underfills the chip
// (< ~1.5 blocks/CU), halve the narrower output dim's tile.
constexpr long long kDenseNarrowTiles = 384;
// Split-K tile geometry: 128x128 has 2x the arithmetic intensity of the
// narrow tiles and the K-split supplies the grid fill, so it wins whenever
// the chip can be covered at all (measured +45..100% on the BERT wgrad
// shapes, BERT end-to-end +12%); narrow geometries only when even max
// splits cannot reach 256 blocks, 128x32 for the skinny-N LoRA shapes.
constexpr long long kSplitKNarrowBlocks = 256;
// split K to fill ~2 blocks/CU
constexpr long long kSplitKTargetBlocks = 512;

inline int gemm_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// 2-phase tile: 128x32 for N <= 32 (skinny adapters / LoRA), else 128x128,
// or with `narrow` the narrower output dim's tile halved (128x64 / 64x128).
inline void gemm_set_tile(GemmPlan& pl, bool narrow, int M, int N, int gz) {
  narrow = narrow && N > 32;
  pl.bm = narrow && N > M ? 64 : 128;
  pl.bn = N <= 32 ? 32 : (narrow && N <= M ? 64 : 128);
  pl.grid_x = gemm_cdiv(N, pl.bn);
  pl.grid_y = gemm_cdiv(M, pl.bm);
  pl.grid_z = gz;
}

// 8-wave kernels: full 256x256 tiles only
inline void gemm_set_tile8(GemmPlan& pl, int M, int N, int gz) {
  pl.bm = pl.bn = kTile8;
  pl.grid_x = N / kTile8;
  pl.grid_y = M / kTile8;
  pl.grid_z = gz;
}

// Slab split count for t256 output tiles of 256x256 over contraction K:
// double while the blocks fit and the slices stay long; 1 = no slab route
// (nothing to split, or the slice is not a whole number of 32-wide k-halves).
inline int slab_splits(long long t256, int K) {
  int s = 1;
  while ((long long)s * 2 * t256 <= kSlabMaxBlocks && K % (s * 2) == 0 &&
         K / (s * 2) >= kSlabMinChunk)
    s *= 2;
  return (K / s) % 32 == 0 ? s : 1;
}

// 8-phase split-K with per-slice slabs + reduce (no fp32 atomics — the
// atomic 8-phase variant measured slower, r1 profiles). M, N multiples of
// 256, splits from slab_splits(). g9 walks 64-wide K-tiles, so a slice
// with an odd number of 32-wide k-halves takes the g8 kernel.
inline GemmPlan plan_slab(int M, int N, int K, int splits) {
  GemmPlan pl{};
  pl.k_chunk = K / splits;
  pl.kind = pl.k_chunk % 64 == 0 ? GemmKind::G9Slab : GemmKind::G8Slab;
  pl.splits = splits;
  gemm_set_tile8(pl, M, N, splits);
  pl.use_swz = 1;
  pl.m_main = M;
  return pl;
}

// 2-phase split-K (an 8-phase split-K variant with ATOMICS was measured
// slower here: the 256^2 tile quadruples each block's fp32 atomic output
// volume — see profiles/; the 128^2 2-phase split-K wins for these shapes)
inline GemmPlan plan_splitk(int layout, int M, int N, int K) {
  GemmPlan pl{};
  pl.layout = layout;
  pl.kind = GemmKind::TwoPhaseSplitK;
  const long long tiles128 = (long long)gemm_cdiv(M, 128) * gemm_cdiv(N, 128);
  gemm_set_tile(pl, tiles128 * gemm_cdiv(K, kGemmBK) < kSplitKNarrowBlocks, M,
                N, 1);
  const long long tiles = (long long)pl.grid_x * pl.grid_y;
  int splits = (int)(kSplitKTargetBlocks / (tiles > 0 ? tiles : 1));
  if (splits < 1) splits = 1;
  const int max_splits = gemm_cdiv(K, kGemmBK);
  if (splits > max_splits) splits = max_splits;
  pl.k_chunk = gemm_cdiv(gemm_cdiv(K, splits), kGemmBK) * kGemmBK;
  pl.grid_z = pl.splits = gemm_cdiv(K, pl.k_chunk);
  pl.m_main = M;
  return pl;
}

// No re-layout, no K split: the route of the batched / strided entry
// points, and of gemm() once plan_gemm() has ruled the others out.
inline GemmPlan plan_dense(const GemmProblem& p) {
  GemmPlan pl{};
  pl.layout = p.layout;
  pl.splits = 1;
  pl.k_chunk = p.K;
  pl.m_main = p.M;
  const long long op_bytes = ((long long)p.M * p.K + (long long)p.N * p.K) *
                             (p.bf16 ? 2 : 4) * p.nbatch;
  pl.use_swz = op_bytes > kSwizzleBytes ? 1 : 0;
  // Deep-pipelined 256x256 8-wave kernel for big bf16 NT tiles (gemm8.hip;
  // fp32 bias is fused in its epilogue). Ragged M (e.g. token counts): run
  // the 256-aligned row block on the deep kernel and the remainder rows on
  // the 2-phase kernel.
  if (p.bf16 && !p.out_f32 && p.layout == 0 && !p.relu && p.nbatch == 1 &&
      (float)p.beta == 0.f && !p.strided && p.N % kTile8 == 0 &&
      p.K % 64 == 0 &&
      (long long)(p.M / kTile8) * (p.N / kTile8) >= kG9MinBlocks) {
    pl.kind = GemmKind::G9;
    pl.m_main = p.M / kTile8 * kTile8;
    gemm_set_tile8(pl, p.M, p.N, 1);
    return pl;
  }
  pl.kind = GemmKind::TwoPhase;
  const long long tiles128 =
      (long long)gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, 128) * p.nbatch;
  gemm_set_tile(pl, tiles128 < kDenseNarrowTiles, p.M, p.N, p.nbatch);
  return pl;
}

// The rows a ragged-M G9 plan leaves over, as a problem of their own
// (A and C advance by pl.m_main rows; B and bias are shared), in the
// plan's layout: any re-layout is done by then.
inline GemmProblem gemm_remainder(GemmProblem p, const GemmPlan& pl) {
  p.M -= pl.m_main;
  p.layout = pl.layout;
  return p;
}

// gemm(): the glds NT path is the fast one, so big transposed operands are
// re-laid-out once; small-tile long-K cases split the contraction over
// grid.z with fp32 accumulation. `direct` skips the transpose-to-NT
// re-layouts (split-K still applies): for a skinny-M NN like the LoRA dB^T
// (= xa^T @ dz), transposing the big [tokens, out] upstream grad costs more
// than the NT gain.
inline GemmPlan plan_gemm(const GemmProblem& p) {
  const bool plain = p.beta == 0.0 && !p.has_bias && !p.relu;
  bool ta = false, tb = false;
  if (!p.direct && plain && p.layout == 2 && !p.out_f32) {
    // TN -> NT: transpose both (any shape; bounds handled by staging)
    ta = tb = true;
  } else if (!p.direct && plain && p.layout == 1 &&
             (long long)p.K * p.N * (p.bf16 ? 2 : 4) >= kNNTransposeBytes) {
    tb = true;   // big NN: transpose B -> NT
  }
  // layout 2 survives only with `direct` or out_f32: native-TN, no transposes
  const int layout = (ta || tb) ? 0 : p.layout;
  GemmPlan pl;
  const long long tiles =
      (long long)gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, p.N <= 32 ? 32 : 128);
  if (plain && p.alpha == 1.0 && tiles < kSplitKMaxTiles &&
      p.K >= kSplitKMinK) {
    // Slab route covers the long-K skinny-tile wgrads (BERT dW:
    // 256-divisible M/N).
    int splits = 1;
    if (layout == 0 && p.bf16 && p.M % kTile8 == 0 && p.N % kTile8 == 0)
      splits = slab_splits((long long)(p.M / kTile8) * (p.N / kTile8), p.K);
    pl = splits > 1 ? plan_slab(p.M, p.N, p.K, splits)
                    : plan_splitk(layout, p.M, p.N, p.K);
  } else {
    GemmProblem q = p;
    q.layout = layout;
    pl = plan_dense(q);
  }
  pl.layout = layout;
  pl.transpose_a = ta;
  pl.transpose_b = tb;
  return pl;
}

// Epilogue / layout combinations the dense launch ladder (launch_dense in
// gemm.hip) has no instantiation for: the reason, or nullptr when `pl` (the
// plan of `p`) can run. The fp32-output bf16 kernel exists for TN only and
// the relu epilogue for NT only; launched anyway, the first would write bf16
// into an fp32 buffer and the second would drop the relu. The split routes
// accumulate in fp32 for every layout, so out_f32 is fine there, and with
// fp32 inputs it changes nothing.
inline const char* gemm_unsupported(const GemmProblem& p, const GemmPlan& pl) {
  const bool dense = pl.kind == GemmKind::TwoPhase || pl.kind == GemmKind::G9;
  if (p.out_f32 && p.bf16 && dense && pl.layout != 2)
    return "out_f32 with bf16 inputs on the dense route is TN-only";
  if (p.relu && pl.layout != 0) return "the relu epilogue is NT-only";
  return nullptr;
}

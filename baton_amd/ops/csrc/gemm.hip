// MFMA GEMM kernels (gfx950) — the Linear-layer hot path and the base of
// the attention path.
//
// From-scratch CDNA4 design (the reference's only GEMM is CPU nn.Linear,
// /root/reference/demo.py:23):
//   * v_mfma_f32_16x16x32_bf16 (bf16 in, fp32 acc) / v_mfma_f32_16x16x4_f32
//     (exact f32 — no TF32 on gfx950);
//   * tile geometry templated: 128x128 (2x2 waves), 128x64 (4x1), 64x128
//     (1x4), 128x32 (4x1) — gemm_plan.h picks whichever fills 256 CUs;
//   * DOUBLE-BUFFERED LDS, one barrier per K-step (2-phase pipeline);
//   * bf16 staging uses __builtin_amdgcn_global_load_lds (16-B direct
//     HBM->LDS DMA, no VGPR round-trip) on full interior tiles. glds
//     writes lane-linear, so the LDS image is LINEAR (no pad) and bank
//     conflicts are killed by a slot XOR swizzle applied on BOTH the
//     per-lane global SOURCE address and the ds_read offsets (guide rule
//     21: dest stays linear). Layout: 64-B rows (BK=32 bf16), 16-B slot
//     s at row r lives at physical slot s ^ ((r>>2)&3) — the 16-lane
//     ds_read_b128 fragment groups then touch 16 distinct slots per 256-B
//     bank row (conflict-free);
//   * edge tiles / transposed operands fall back to register staging that
//     writes the same swizzled image; fp32 uses a padded layout (+2
//     elements) with scalar b32 fragment reads;
//   * batched via grid.z (attention: one batch per B*H);
//   * TN split-K variant for Linear wgrad (small output, long contraction).
#include "common.h"

constexpr int BK = 32;
constexpr int FRAG = 16;

// LDS layout helpers (lds_off / lds_row_elems) live in common.h.

// ---- staging ---------------------------------------------------------------
// Canonical image: rows = output-dim (M or N), cols = K slice (k-contig).

// direct: source row-major [rows][K] -> vector loads; writes swizzled image.
template <typename T, int ROWS>
DEVINL void stage_direct(T* __restrict__ lds, const T* __restrict__ src,
                         long long ld, int row0, int k0, int rows_limit,
                         int k_limit) {
  constexpr int ELEMS = 16 / sizeof(T);
  constexpr int THREADS_PER_ROW = BK / ELEMS;
  constexpr int TOTAL = ROWS * THREADS_PER_ROW;       // vector slots in tile
  using VT = typename VecTraits<T>::VecT;
#pragma unroll
  for (int p = 0; p < (TOTAL + kBlock - 1) / kBlock; ++p) {
    int idx = p * kBlock + threadIdx.x;
    if (idx >= TOTAL) break;
    int row = idx / THREADS_PER_ROW;
    int kc = (idx % THREADS_PER_ROW) * ELEMS;
    VT v;
    T* vp = reinterpret_cast<T*>(&v);
    if (row0 + row < rows_limit && k0 + kc + ELEMS <= k_limit) {
      v = *reinterpret_cast<const VT*>(&src[(long long)(row0 + row) * ld + k0 + kc]);
    } else {
#pragma unroll
      for (int j = 0; j < ELEMS; ++j)
        vp[j] = (row0 + row < rows_limit && k0 + kc + j < k_limit)
                    ? src[(long long)(row0 + row) * ld + k0 + kc + j]
                    : (T)0.f;
    }
    *reinterpret_cast<VT*>(&lds[lds_off<T>(row, kc)]) = v;
  }
}

// glds: bf16 full tiles with 16-B-alignable rows. The hardware writes lane
// l's 16 B at (wave-uniform base) + l*16, so the swizzle is applied to the
// SOURCE address each lane loads from.
DEVINL void stage_direct_glds(bf16* __restrict__ lds, const bf16* __restrict__ src,
                              long long ld, int row0, int k0, int rows) {
  const int t = threadIdx.x;
  const int w = t >> 6;                  // wave id (uniform per wave)
  const int total = rows * 4;            // 16-B slots in the tile
  for (int p = 0; p * kBlock < total; ++p) {
    const int idx = p * kBlock + t;
    if (idx >= total) break;             // whole waves drop out together
    const int row = idx >> 2;                // 4 slots per row
    const int psl = idx & 3;                 // physical slot this lane fills
    const int lsl = psl ^ ((row >> 2) & 3);  // logical slot -> source k
    auto g = (const __attribute__((address_space(1))) unsigned int*)(
        src + (long long)(row0 + row) * ld + k0 + lsl * 8);
    // wave-uniform LDS base: this wave's 64 lanes fill 1 KiB linearly
    auto l = (__attribute__((address_space(3))) unsigned int*)(
        lds + (long long)(p * kBlock + w * 64) * 8);
    __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0);
  }
}

// transposed: source row-major [K][rows] -> vector load along rows, scatter
// scalar writes into the (swizzled/padded) image.
template <typename T, int ROWS>
DEVINL void stage_transposed(T* __restrict__ lds, const T* __restrict__ src,
                             long long ld, int row0, int k0, int rows_limit,
                             int k_limit) {
  constexpr int ELEMS = 16 / sizeof(T);
  constexpr int VECS_PER_K = ROWS / ELEMS;
  using VT = typename VecTraits<T>::VecT;
  constexpr int TOTAL = BK * VECS_PER_K;
#pragma unroll
  for (int p = 0; p < (TOTAL + kBlock - 1) / kBlock; ++p) {
    int idx = p * kBlock + threadIdx.x;
    if (idx >= TOTAL) break;
    int k = idx % BK;
    int r = (idx / BK) * ELEMS;
    VT v;
    T* vp = reinterpret_cast<T*>(&v);
    if (k0 + k < k_limit && row0 + r + ELEMS <= rows_limit) {
      v = *reinterpret_cast<const VT*>(&src[(long long)(k0 + k) * ld + row0 + r]);
    } else {
#pragma unroll
      for (int j = 0; j < ELEMS; ++j)
        vp[j] = (k0 + k < k_limit && row0 + r + j < rows_limit)
                    ? src[(long long)(k0 + k) * ld + row0 + r + j]
                    : (T)0.f;
    }
#pragma unroll
    for (int j = 0; j < ELEMS; ++j) lds[lds_off<T>(r + j, k)] = vp[j];
  }
}

// ---- MFMA over one staged K-step -------------------------------------------

template <typename T, int MF, int NF>
DEVINL void gemm_mma(const T* a_lds, const T* b_lds, f32x4 (&acc)[MF][NF],
                     int lane, int wm0, int wn0) {
  if constexpr (sizeof(T) == 2) {
    s16x8 a_frag[MF], b_frag[NF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
      a_frag[mf] = *reinterpret_cast<const s16x8*>(
          &a_lds[lds_off<T>(wm0 + mf * FRAG + (lane & 15), (lane >> 4) * 8)]);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
      b_frag[nf] = *reinterpret_cast<const s16x8*>(
          &b_lds[lds_off<T>(wn0 + nf * FRAG + (lane & 15), (lane >> 4) * 8)]);
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[mf], b_frag[nf], acc[mf][nf], 0, 0, 0);
  } else {
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      float a_s[MF], b_s[NF];
      const int kidx = kk * 4 + (lane >> 4);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        a_s[mf] = ((const float*)a_lds)[lds_off<T>(wm0 + mf * FRAG + (lane & 15), kidx)];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        b_s[nf] = ((const float*)b_lds)[lds_off<T>(wn0 + nf * FRAG + (lane & 15), kidx)];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a_s[mf], b_s[nf], acc[mf][nf], 0, 0, 0);
    }
  }
}

// ---- the kernel ------------------------------------------------------------
// C[M,N] = alpha * op(A) @ op(B) + beta * C (+ bias[n]) (+ relu)
//   TA=0: A[M,K] row-major; TA=1: A[K,M] row-major.
//   TB=0: B[K,N] row-major; TB=1: B[N,K] row-major.

template <typename T, typename TOUT, bool TA, bool TB, bool RELU,
          int BM_, int BN_, int WAVES_M, int WAVES_N, bool SPLITK>
__global__ __launch_bounds__(kBlock) void gemm_kernel(
    const T* __restrict__ A, const T* __restrict__ B, TOUT* __restrict__ C,
    const float* __restrict__ bias, int M, int N, int K, float alpha,
    float beta, long long strideA, long long strideB, long long strideC,
    int k_chunk, int use_swz, int b_group, GemmStrides gs) {
  constexpr int WM = BM_ / WAVES_M;
  constexpr int WN = BN_ / WAVES_N;
  constexpr int MF = WM / FRAG;
  constexpr int NF = WN / FRAG;
  constexpr int RE = lds_row_elems<T>();
  // ONE shared object (glds pipelines de-schedule with several — guide
  // §5 trap (a)); [buffer][A image | B image].
  __shared__ T lds_all[2 * (BM_ + BN_) * RE];
  auto a_lds = [&](int buf) -> T* { return lds_all + buf * (BM_ + BN_) * RE; };
  auto b_lds = [&](int buf) -> T* {
    return lds_all + buf * (BM_ + BN_) * RE + BM_ * RE;
  };

  if (gs.heads > 1) {
    // two-level batch: z = outer * heads + head (strided attention views)
    const long long zo = blockIdx.z / gs.heads;
    const long long zi = blockIdx.z % gs.heads;
    A += zo * strideA + zi * gs.a2;
    B += zo * strideB + (zi / b_group) * gs.b2;   // GQA on the head index
    C += zo * strideC + zi * gs.c2;
  } else {
    A += (long long)blockIdx.z * strideA;
    // b_group > 1: GQA — b_group consecutive batches share one B (KV head)
    B += (long long)(blockIdx.z / b_group) * strideB;
    C += (long long)blockIdx.z * strideC;
  }
  const int bid = xcd_block_id(use_swz);
  const int tile_n = bid % gridDim.x, tile_m2 = bid / gridDim.x;
  const int m0 = tile_m2 * BM_, n0 = tile_n * BN_;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int wm0 = (wid / WAVES_N) * WM;
  const int wn0 = (wid % WAVES_N) * WN;

  f32x4 acc[MF][NF] = {};

  const long long lda = gs.lda ? gs.lda : (TA ? M : K);
  const long long ldb = gs.ldb ? gs.ldb : (TB ? K : N);
  const long long ldc = gs.ldc ? gs.ldc : N;
  // glds eligibility (bf16, full tile, 16-B-aligned rows)
  const bool glds_a = sizeof(T) == 2 && !TA && (m0 + BM_ <= M) && (lda % 8 == 0);
  const bool glds_b = sizeof(T) == 2 && TB && (n0 + BN_ <= N) && (ldb % 8 == 0);

  auto stage = [&](int buf, int k0) {
    const bool k_full = (k0 + BK <= K);
    if (TA) {
      stage_transposed<T, BM_>(a_lds(buf), A, lda, m0, k0, M, K);
    } else if (glds_a && k_full) {
      if constexpr (sizeof(T) == 2)
        stage_direct_glds((bf16*)a_lds(buf), (const bf16*)A, lda, m0, k0, BM_);
    } else {
      stage_direct<T, BM_>(a_lds(buf), A, lda, m0, k0, M, K);
    }
    if (TB) {
      if (glds_b && k_full) {
        if constexpr (sizeof(T) == 2)
          stage_direct_glds((bf16*)b_lds(buf), (const bf16*)B, ldb, n0, k0, BN_);
      } else {
        stage_direct<T, BN_>(b_lds(buf), B, ldb, n0, k0, N, K);
      }
    } else {
      stage_transposed<T, BN_>(b_lds(buf), B, ldb, n0, k0, N, K);
    }
  };

  // SPLITK: this block covers K slice [k_begin, k_end)
  const int k_begin = SPLITK ? blockIdx.z * k_chunk : 0;
  const int k_end = SPLITK ? min(k_begin + k_chunk, K) : K;
  const int nk = (k_end - k_begin + BK - 1) / BK;
  if (nk <= 0) return;
  stage(0, k_begin);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(cur ^ 1, k_begin + (kt + 1) * BK);
    gemm_mma<T, MF, NF>(a_lds(cur), b_lds(cur), acc, lane, wm0, wn0);
    __syncthreads();
  }

  // Epilogue. C/D fragment map: col = lane&15, row = (lane>>4)*4 + r.
  const int col_in_frag = lane & 15;
  const int row_base = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm0 + mf * FRAG + row_base + r;
        int col = n0 + wn0 + nf * FRAG + col_in_frag;
        if (row < M && col < N) {
          long long off = (long long)row * ldc + col;
          float v = alpha * acc[mf][nf][r];
          if (SPLITK) {
            // fp32 atomic accumulation across K slices (TOUT = float)
            if (gridDim.z == 1)
              C[off] = (TOUT)v;
            else
              atomicAdd((float*)&C[off], v);
          } else {
            if (beta != 0.f) v = fmaf(beta, (float)C[off], v);
            if (bias != nullptr) v += bias[col];
            if (RELU) v = fmaxf(v, 0.f);
            C[off] = (TOUT)v;
          }
        }
      }
    }
  }
}

// ---- launchers -------------------------------------------------------------
// Launch exactly the kernel a GemmPlan (gemm_plan.h) names; every routing
// decision lives in the planner. A false return means the plan does not fit
// the problem and nothing was launched.
#include "launchers.h"

namespace {

template <int BM_, int BN_, int WAVES_M_, int WAVES_N_>
struct Geom {
  static constexpr int BM = BM_, BN = BN_, WAVES_M = WAVES_M_, WAVES_N = WAVES_N_;
};

// The one tile-geometry ladder: the instantiated tiles and their wave grids.
template <typename F>
bool with_geom(int bm, int bn, F&& f) {
  if (bm == 128 && bn == 128) f(Geom<128, 128, 2, 2>{});
  else if (bm == 128 && bn == 64) f(Geom<128, 64, 4, 1>{});
  else if (bm == 64 && bn == 128) f(Geom<64, 128, 1, 4>{});
  else if (bm == 128 && bn == 32) f(Geom<128, 32, 4, 1>{});
  else return false;
  return true;
}

struct GemmArgs {
  const void *A, *B;
  void* C;
  const float* bias;
  int M, N, K;
  float alpha, beta;
  long long strideA, strideB, strideC;
  int b_group;
  GemmStrides gs;
};

template <typename T, typename TOUT, bool TA, bool TB, bool RELU,
          bool SPLITK = false>
bool launch_tile(const GemmPlan& pl, const GemmArgs& a, hipStream_t s) {
  return with_geom(pl.bm, pl.bn, [&](auto g) {
    using G = decltype(g);
    hipLaunchKernelGGL(
        (gemm_kernel<T, TOUT, TA, TB, RELU, G::BM, G::BN, G::WAVES_M,
                     G::WAVES_N, SPLITK>),
        dim3(pl.grid_x, pl.grid_y, pl.grid_z), dim3(kBlock), 0, s,
        (const T*)a.A, (const T*)a.B, (TOUT*)a.C, a.bias, a.M, a.N, a.K,
        a.alpha, a.beta, a.strideA, a.strideB, a.strideC,
        SPLITK ? pl.k_chunk : 0, pl.use_swz, a.b_group, a.gs);
  });
}

// Layout ladders: NT (fwd), NN (dgrad), TN (wgrad, bf16 also with fp32 out).
template <typename T>
bool launch_dense(const GemmPlan& pl, bool out_f32, bool relu,
                  const GemmArgs& a, hipStream_t s) {
  if (pl.layout == 0)
    return relu ? launch_tile<T, T, false, true, true>(pl, a, s)
                : launch_tile<T, T, false, true, false>(pl, a, s);
  if (pl.layout == 1) return launch_tile<T, T, false, false, false>(pl, a, s);
  return out_f32 ? launch_tile<T, float, true, false, false>(pl, a, s)
                 : launch_tile<T, T, true, false, false>(pl, a, s);
}

template <typename T>
bool launch_splitk(const GemmPlan& pl, const GemmArgs& a, hipStream_t s) {
  if (pl.layout == 0)
    return launch_tile<T, float, false, true, false, true>(pl, a, s);
  if (pl.layout == 1)
    return launch_tile<T, float, false, false, false, true>(pl, a, s);
  return launch_tile<T, float, true, false, false, true>(pl, a, s);
}

// the plan's grid must cover the output exactly once
bool grid_fits(const GemmPlan& pl, int M, int N, int gz) {
  return pl.bm > 0 && pl.bn > 0 && pl.grid_x == (N + pl.bn - 1) / pl.bn &&
         pl.grid_y == (M + pl.bm - 1) / pl.bm && pl.grid_z == gz;
}

}  // namespace

bool launch_gemm_2ph(const GemmPlan& pl, const GemmProblem& p, const void* A,
                     const void* B, void* C, const float* bias,
                     long long strideA, long long strideB, long long strideC,
                     hipStream_t s, int b_group, GemmStrides gs) {
  if (pl.kind != GemmKind::TwoPhase || !grid_fits(pl, p.M, p.N, p.nbatch))
    return false;
  const GemmArgs a{A, B, C, bias, p.M, p.N, p.K, (float)p.alpha, (float)p.beta,
                   strideA, strideB, strideC, b_group, gs};
  return p.bf16 ? launch_dense<bf16>(pl, p.out_f32, p.relu, a, s)
                : launch_dense<float>(pl, p.out_f32, p.relu, a, s);
}

bool launch_gemm_2ph_splitk(const GemmPlan& pl, bool in_bf16, const void* A,
                            const void* B, float* C, int M, int N, int K,
                            hipStream_t s) {
  // the K slices must tile [0, K) in whole K-steps
  if (pl.kind != GemmKind::TwoPhaseSplitK || !grid_fits(pl, M, N, pl.splits) ||
      pl.splits < 1 || pl.k_chunk < BK || pl.k_chunk % BK != 0 ||
      (long long)pl.splits * pl.k_chunk < K ||
      (long long)(pl.splits - 1) * pl.k_chunk >= K)
    return false;
  const GemmArgs a{A, B, C, nullptr, M, N, K, 1.f, 0.f, 0, 0, 0, 1,
                   GemmStrides{0, 0, 0, 1, 0, 0, 0}};
  return in_bf16 ? launch_splitk<bf16>(pl, a, s) : launch_splitk<float>(pl, a, s);
}

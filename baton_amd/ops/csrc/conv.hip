// Implicit-GEMM convolution (gfx950), NHWC layout, forward + dgrad + wgrad.
//
// Required by the ResNet federated configs (SURVEY.md §2.2 row
// "Conv/BatchNorm"; the reference has no conv at all). The convolution IS
// a GEMM on MFMA — no im2col materialization; A/B tiles are gathered
// straight from NHWC tensors into LDS.
//
// Performance structure:
//   * tiles TEMPLATED: 128x128 (2x2 waves), 128x64 (4x1) when the output
//     channel dim is <= 64 (stem/layer1), 64x128 (1x4) for wgrad of
//     64-filter layers;
//   * DOUBLE-BUFFERED LDS, one barrier per k-step;
//   * STATEFUL STAGERS: the pixel decode (m -> n,ho,wo — integer div/mod)
//     is hoisted out of the K-loop (it is k-invariant), and the tap walk
//     (ci,kw,kh / co,kw,kh) advances INCREMENTALLY by CBK per staged tile
//     — the hot loop has no integer division at all on the fast path
//     (channels % 32 == 0, i.e. every ResNet layer but the stem);
//   * stride-2 dgrad is PHASE-DECOMPOSED (dgrad_phase_map.h): M tiles per
//     input-parity class, K loop over that class's live taps only;
//   * wgrad splits the pixel contraction over grid.z (fp32 atomics);
//   * LDS rows padded +8 elements: conflict-free ds_read_b128 groups.
#include "common.h"
#include "dgrad_phase_map.h"

constexpr int CBK = 32;
constexpr int CFRAG = 16;

struct ConvShape {
  int N, H, W, Cin, Cout, KH, KW, stride, pad, HO, WO, swz;
};

// ---- stateful stagers ------------------------------------------------------


// bf16 glds staging of a [ROWS][32] K-slice (linear+swizzled image; the
// swizzle rides on each lane's SOURCE address). Only callable when every
// lane's 16 B is in bounds: full row tile, k-slice inside K, rows 16-B
// alignable (ld % 8 == 0).
template <int ROWS>
DEVINL void stage_glds_rows(bf16* __restrict__ lds, const bf16* __restrict__ src,
                            long long ld, long long row0, int k0) {
  const int t = threadIdx.x;
  const int w = t >> 6;
  constexpr int TOTAL = ROWS * 4;          // 16-B slots
#pragma unroll
  for (int p = 0; p * kBlock < TOTAL; ++p) {
    const int idx = p * kBlock + t;
    if (idx >= TOTAL) break;               // whole waves drop out together
    const int row = idx >> 2;
    const int psl = idx & 3;
    const int lsl = psl ^ ((row >> 2) & 3);
    auto g = (const __attribute__((address_space(1))) unsigned int*)(
        src + (row0 + row) * ld + k0 + lsl * 8);
    auto l = (__attribute__((address_space(3))) unsigned int*)(
        lds + (long long)(p * kBlock + w * 64) * 8);
    __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0);
  }
}

// Forward A: rows = output pixels, k = (kh,kw,ci), FAST = Cin % 32 == 0.
template <typename T, int ROWS, bool FAST>
struct FwdAStager {
  static constexpr int ELEMS = 16 / (int)sizeof(T);
  static constexpr int TPR = CBK / ELEMS;           // threads per row
  static constexpr int RPP = kBlock / TPR;          // rows per pass
  static constexpr int PASSES = ROWS / RPP;
  int kc;                                           // k offset of this thread
  int row[PASSES];
  int n[PASSES], ho[PASSES], wo[PASSES];
  bool ok[PASSES];
  int ci, kw, kh;                                   // FAST tap state
  int k_generic;                                    // generic-path k cursor
  int m0_;                                          // tile base row
  bool full_;                                       // whole tile in bounds

  DEVINL void init(const ConvShape& sh, int m0, int Mtot) {
    m0_ = m0;
    full_ = (m0 + ROWS <= Mtot);
    kc = (threadIdx.x % TPR) * ELEMS;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      row[p] = p * RPP + threadIdx.x / TPR;
      const int m = m0 + row[p];
      wo[p] = m % sh.WO;
      const int t = m / sh.WO;
      ho[p] = t % sh.HO;
      n[p] = t / sh.HO;
      ok[p] = m < Mtot;
    }
    ci = kc;     // FAST: Cin >= 32, so k=kc decodes to tap 0, channel kc
    kw = 0;
    kh = 0;
    k_generic = kc;
  }

  // stage one k-tile (called once per tile, ascending), then advance state
  DEVINL void stage(T* __restrict__ lds, const T* __restrict__ x,
                    const ConvShape& sh, int Ktot) {
    using VT = typename VecTraits<T>::VecT;
    if constexpr (sizeof(T) == 2 && FAST) {
      // 1x1 stride-1 conv on a full pixel tile IS a dense GEMM slice
      // (block-uniform condition: the whole 128-pixel tile is in bounds).
      // ci carries the PER-THREAD scalar-path offset kc; the glds helper
      // wants the block-uniform tile base, so strip kc back out.
      // A 1xKW kernel or a padded 1x1 is NOT one: its rows are shifted /
      // padded pixels, and its output has more rows than x has pixels.
      if (sh.KH == 1 && sh.KW == 1 && sh.pad == 0 && sh.stride == 1 && full_ &&
          (sh.Cin % 8) == 0) {
        stage_glds_rows<ROWS>((bf16*)lds, (const bf16*)x, sh.Cin,
                              (long long)m0_, ci - kc);
        ci += CBK;
        if (ci >= sh.Cin) {
          ci -= sh.Cin;
          if (++kw == sh.KW) { kw = 0; ++kh; }
        }
        return;
      }
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      VT v;
      T* vp = reinterpret_cast<T*>(&v);
      if (FAST) {
        const int hi = ho[p] * sh.stride - sh.pad + kh;
        const int wi = wo[p] * sh.stride - sh.pad + kw;
        if (ok[p] && hi >= 0 && hi < sh.H && wi >= 0 && wi < sh.W) {
          v = *reinterpret_cast<const VT*>(
              &x[(((long long)n[p] * sh.H + hi) * sh.W + wi) * sh.Cin + ci]);
        } else {
#pragma unroll
          for (int j = 0; j < ELEMS; ++j) vp[j] = (T)0.f;
        }
      } else {
#pragma unroll
        for (int j = 0; j < ELEMS; ++j) {
          const int k = k_generic + j;
          vp[j] = (T)0.f;
          if (ok[p] && k < Ktot) {
            const int cij = k % sh.Cin, tap = k / sh.Cin;
            const int kwj = tap % sh.KW, khj = tap / sh.KW;
            const int hi = ho[p] * sh.stride - sh.pad + khj;
            const int wi = wo[p] * sh.stride - sh.pad + kwj;
            if (hi >= 0 && hi < sh.H && wi >= 0 && wi < sh.W)
              vp[j] = x[(((long long)n[p] * sh.H + hi) * sh.W + wi) * sh.Cin + cij];
          }
        }
      }
      *reinterpret_cast<VT*>(&lds[lds_off<T>(row[p], kc)]) = v;
    }
    if (FAST) {
      ci += CBK;
      if (ci >= sh.Cin) {
        ci -= sh.Cin;
        if (++kw == sh.KW) { kw = 0; ++kh; }
      }
    } else {
      k_generic += CBK;
    }
  }
};

// Direct row-major K-contiguous staging (forward B / dgrad B from w_t /
// wgrad A from dy_t): glds for full bf16 tiles, register staging otherwise.
// ld = source row length (may exceed k_limit for split-K pixel slices).
template <typename T, int ROWS>
DEVINL void stage_fwd_B(T* __restrict__ lds, const T* __restrict__ w,
                        int n0, int k0, int Ntot, int k_limit,
                        long long ld) {
  if constexpr (sizeof(T) == 2) {
    if (n0 + ROWS <= Ntot && k0 + CBK <= k_limit && (ld % 8) == 0) {
      stage_glds_rows<ROWS>((bf16*)lds, (const bf16*)w, ld, n0, k0);
      return;
    }
  }
  constexpr int ELEMS = 16 / sizeof(T);
  constexpr int TPR = CBK / ELEMS;
  constexpr int RPP = kBlock / TPR;
  using VT = typename VecTraits<T>::VecT;
#pragma unroll
  for (int p = 0; p < ROWS / RPP; ++p) {
    int idx = p * kBlock + threadIdx.x;
    int row = idx / TPR;
    int kc = (idx % TPR) * ELEMS;
    VT v;
    T* vp = reinterpret_cast<T*>(&v);
    if (n0 + row < Ntot && k0 + kc + ELEMS <= k_limit) {
      v = *reinterpret_cast<const VT*>(&w[(long long)(n0 + row) * ld + k0 + kc]);
    } else {
#pragma unroll
      for (int j = 0; j < ELEMS; ++j)
        vp[j] = (n0 + row < Ntot && k0 + kc + j < k_limit)
                    ? w[(long long)(n0 + row) * ld + k0 + kc + j]
                    : (T)0.f;
    }
    *reinterpret_cast<VT*>(&lds[lds_off<T>(row, kc)]) = v;
  }
}

// dgrad A: rows = input pixels, k = (kh,kw,co), FAST = Cout % 32 == 0.
template <typename T, int ROWS, bool FAST>
struct DgradAStager {
  static constexpr int ELEMS = 16 / (int)sizeof(T);
  static constexpr int TPR = CBK / ELEMS;
  static constexpr int RPP = kBlock / TPR;
  static constexpr int PASSES = ROWS / RPP;
  int kc;
  int n[PASSES], hq[PASSES], wq[PASSES];
  bool ok[PASSES];
  int co, kw, kh;
  int k_generic;

  DEVINL void init(const ConvShape& sh, int m0, int Mtot) {
    kc = (threadIdx.x % TPR) * ELEMS;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int q = m0 + p * RPP + threadIdx.x / TPR;
      wq[p] = q % sh.W;
      const int t = q / sh.W;
      hq[p] = t % sh.H;
      n[p] = t / sh.H;
      ok[p] = q < Mtot;
    }
    co = kc;
    kw = 0;
    kh = 0;
    k_generic = kc;
  }

  DEVINL void stage(T* __restrict__ lds, const T* __restrict__ dy,
                    const ConvShape& sh, int Ktot) {
    using VT = typename VecTraits<T>::VecT;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      VT v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int j = 0; j < ELEMS; ++j) vp[j] = (T)0.f;
      if (FAST) {
        if (ok[p]) {
          const int hnum = hq[p] + sh.pad - kh, wnum = wq[p] + sh.pad - kw;
          if (hnum >= 0 && wnum >= 0 && hnum % sh.stride == 0 &&
              wnum % sh.stride == 0) {
            const int ho = hnum / sh.stride, wo = wnum / sh.stride;
            if (ho < sh.HO && wo < sh.WO)
              v = *reinterpret_cast<const VT*>(
                  &dy[(((long long)n[p] * sh.HO + ho) * sh.WO + wo) * sh.Cout + co]);
          }
        }
      } else if (ok[p]) {
#pragma unroll
        for (int j = 0; j < ELEMS; ++j) {
          const int k = k_generic + j;
          if (k < Ktot) {
            const int coj = k % sh.Cout, tap = k / sh.Cout;
            const int kwj = tap % sh.KW, khj = tap / sh.KW;
            const int hnum = hq[p] + sh.pad - khj, wnum = wq[p] + sh.pad - kwj;
            if (hnum >= 0 && wnum >= 0 && hnum % sh.stride == 0 &&
                wnum % sh.stride == 0) {
              const int ho = hnum / sh.stride, wo = wnum / sh.stride;
              if (ho < sh.HO && wo < sh.WO)
                vp[j] = dy[(((long long)n[p] * sh.HO + ho) * sh.WO + wo) * sh.Cout + coj];
            }
          }
        }
      }
      *reinterpret_cast<VT*>(&lds[lds_off<T>(p * RPP + threadIdx.x / TPR, kc)]) = v;
    }
    if (FAST) {
      co += CBK;
      if (co >= sh.Cout) {
        co -= sh.Cout;
        if (++kw == sh.KW) { kw = 0; ++kh; }
      }
    } else {
      k_generic += CBK;
    }
  }
};

// Stride-2 dgrad A, one phase class (dgrad_phase_map.h): rows = the class's
// input pixels (n, a, b), k = (the class's taps, co). A tap reads
// dy[n, a + dh, b + dw]: no stride test, only the ho / wo bounds. The tap
// walk itself is block-uniform and lives in the kernel.
template <typename T, int ROWS>
struct DgradPhaseAStager {
  static constexpr int ELEMS = 16 / (int)sizeof(T);
  static constexpr int TPR = CBK / ELEMS;
  static constexpr int RPP = kBlock / TPR;
  static constexpr int PASSES = ROWS / RPP;
  int kc;
  int n[PASSES], a[PASSES], b[PASSES];
  bool ok[PASSES];

  DEVINL void init(const dgph::Class& c, int r0) {
    kc = (threadIdx.x % TPR) * ELEMS;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = r0 + p * RPP + threadIdx.x / TPR;
      const dgph::RowPos pos = dgph::row_pos(c, r);
      n[p] = pos.n; a[p] = pos.a; b[p] = pos.b;
      ok[p] = r < c.rows;
    }
  }

  DEVINL void stage(T* __restrict__ lds, const T* __restrict__ dy,
                    const ConvShape& sh, int dh, int dw, int co0) {
    using VT = typename VecTraits<T>::VecT;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      VT v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int j = 0; j < ELEMS; ++j) vp[j] = (T)0.f;
      const int ho = a[p] + dh, wo = b[p] + dw;
      if (ok[p] && ho >= 0 && ho < sh.HO && wo >= 0 && wo < sh.WO)
        v = *reinterpret_cast<const VT*>(
            &dy[(((long long)n[p] * sh.HO + ho) * sh.WO + wo) * sh.Cout + co0 + kc]);
      *reinterpret_cast<VT*>(&lds[lds_off<T>(p * RPP + threadIdx.x / TPR, kc)]) = v;
    }
  }
};

// wgrad B: rows = (kh,kw,ci) — tap decode HOISTED (k-invariant); the pixel
// (= contraction index) advances incrementally across staged tiles.
template <typename T, int ROWS>
struct WgradBStager {
  static constexpr int ELEMS = 16 / (int)sizeof(T);
  static constexpr int VPK = ROWS / ELEMS;
  static constexpr int TOTAL = CBK * VPK;
  static constexpr int PASSES = (TOTAL + kBlock - 1) / kBlock;
  int k_in_tile[PASSES], rr[PASSES], r_local[PASSES];
  int ci[PASSES], kw[PASSES], kh[PASSES];
  bool active[PASSES], one_tap[PASSES], r_ok[PASSES];
  // pixel state shared across passes with differing k offsets: track per pass
  int wo[PASSES], ho[PASSES], nn[PASSES];
  bool p_ok[PASSES];

  DEVINL void init(const ConvShape& sh, int n0, long long p0, long long p_limit,
                   int Rtot) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int idx = p * kBlock + threadIdx.x;
      active[p] = idx < TOTAL;
      // r-run fastest: consecutive lanes read consecutive 16-B ci runs of
      // the SAME pixel (coalesced gather); pixel-fastest order scattered
      // adjacent lanes a whole pixel stride apart
      k_in_tile[p] = idx / VPK;
      r_local[p] = (idx % VPK) * ELEMS;
      rr[p] = n0 + r_local[p];
      r_ok[p] = rr[p] < Rtot;
      ci[p] = r_ok[p] ? rr[p] % sh.Cin : 0;
      const int tap = r_ok[p] ? rr[p] / sh.Cin : 0;
      kw[p] = tap % sh.KW;
      kh[p] = tap / sh.KW;
      one_tap[p] = (rr[p] / sh.Cin) == ((rr[p] + ELEMS - 1) / sh.Cin);
      const long long px = p0 + k_in_tile[p];
      p_ok[p] = px < p_limit;
      wo[p] = (int)(px % sh.WO);
      const long long t = px / sh.WO;
      ho[p] = (int)(t % sh.HO);
      nn[p] = (int)(t / sh.HO);
    }
  }

  DEVINL void stage(T* __restrict__ lds, const T* __restrict__ x,
                    const ConvShape& sh) {
    using VT = typename VecTraits<T>::VecT;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (!active[p]) continue;
      VT v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int j = 0; j < ELEMS; ++j) vp[j] = (T)0.f;
      if (p_ok[p] && r_ok[p]) {
        if (one_tap[p]) {
          const int hi = ho[p] * sh.stride - sh.pad + kh[p];
          const int wi = wo[p] * sh.stride - sh.pad + kw[p];
          if (hi >= 0 && hi < sh.H && wi >= 0 && wi < sh.W)
            v = *reinterpret_cast<const VT*>(
                &x[(((long long)nn[p] * sh.H + hi) * sh.W + wi) * sh.Cin + ci[p]]);
        } else {
#pragma unroll
          for (int j = 0; j < ELEMS; ++j) {
            const int rj = rr[p] + j;
            const int cij = rj % sh.Cin, tapj = rj / sh.Cin;
            const int kwj = tapj % sh.KW, khj = tapj / sh.KW;
            const int hi = ho[p] * sh.stride - sh.pad + khj;
            const int wi = wo[p] * sh.stride - sh.pad + kwj;
            if (hi >= 0 && hi < sh.H && wi >= 0 && wi < sh.W)
              vp[j] = x[(((long long)nn[p] * sh.H + hi) * sh.W + wi) * sh.Cin + cij];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ELEMS; ++j)
        lds[lds_off<T>(r_local[p] + j, k_in_tile[p])] = vp[j];
      // advance pixel by CBK
      wo[p] += CBK;
      while (wo[p] >= sh.WO) {
        wo[p] -= sh.WO;
        if (++ho[p] == sh.HO) { ho[p] = 0; ++nn[p]; }
      }
    }
  }

  DEVINL void set_p_ok(long long p0, long long p_limit) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) p_ok[p] = (p0 + k_in_tile[p]) < p_limit;
  }
};

// ---- MFMA compute ----------------------------------------------------------

template <typename T, int MF, int NF>
DEVINL void conv_mma(const T* a_lds, const T* b_lds, f32x4 (&acc)[MF][NF],
                     int lane, int wm0, int wn0) {
  if constexpr (sizeof(T) == 2) {
    s16x8 a_frag[MF], b_frag[NF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
      a_frag[mf] = *reinterpret_cast<const s16x8*>(
          &a_lds[lds_off<T>(wm0 + mf * CFRAG + (lane & 15), (lane >> 4) * 8)]);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
      b_frag[nf] = *reinterpret_cast<const s16x8*>(
          &b_lds[lds_off<T>(wn0 + nf * CFRAG + (lane & 15), (lane >> 4) * 8)]);
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[mf], b_frag[nf], acc[mf][nf], 0, 0, 0);
  } else {
#pragma unroll
    for (int kk = 0; kk < CBK / 4; ++kk) {
      float a_s[MF], b_s[NF];
      const int kidx = kk * 4 + (lane >> 4);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        a_s[mf] = ((const float*)a_lds)[lds_off<float>(wm0 + mf * CFRAG + (lane & 15), kidx)];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        b_s[nf] = ((const float*)b_lds)[lds_off<float>(wn0 + nf * CFRAG + (lane & 15), kidx)];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a_s[mf], b_s[nf], acc[mf][nf], 0, 0, 0);
    }
  }
}

// ---- kernels (double-buffered LDS, one barrier per k-step) -----------------

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool FAST>
__global__ __launch_bounds__(kBlock) void conv_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
    ConvShape sh) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MF = WM / CFRAG, NF = WN / CFRAG;
  __shared__ T a_lds[2][BM * lds_row_elems<T>()];
  __shared__ T b_lds[2][BN * lds_row_elems<T>()];
  const int Mtot = sh.N * sh.HO * sh.WO;
  const int Ntot = sh.Cout;
  const int Ktot = sh.KH * sh.KW * sh.Cin;
  // XCD-aware remap (see gemm.hip)
  int t_n, t_m;
  {
    const int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    if (sh.swz && nwg >= 64) {
      const int q = nwg >> 3, r = nwg & 7;
      const int xcd = bid & 7, idx = bid >> 3;
      bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    t_n = bid % gridDim.x;
    t_m = bid / gridDim.x;
  }
  const int m0 = t_m * BM, n0 = t_n * BN;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
  f32x4 acc[MF][NF] = {};
  const int nk = (Ktot + CBK - 1) / CBK;
  FwdAStager<T, BM, FAST> sa;
  sa.init(sh, m0, Mtot);
  sa.stage(a_lds[0], x, sh, Ktot);
  stage_fwd_B<T, BN>(b_lds[0], w, n0, 0, Ntot, Ktot, Ktot);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      sa.stage(a_lds[cur ^ 1], x, sh, Ktot);
      stage_fwd_B<T, BN>(b_lds[cur ^ 1], w, n0, (kt + 1) * CBK, Ntot, Ktot, Ktot);
    }
    conv_mma<T, MF, NF>(a_lds[cur], b_lds[cur], acc, lane, wm0, wn0);
    __syncthreads();
  }
  const int col_in_frag = lane & 15, row_base = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm0 + mf * CFRAG + row_base + r;
        int col = n0 + wn0 + nf * CFRAG + col_in_frag;
        if (row < Mtot && col < Ntot)
          y[(long long)row * Ntot + col] = (T)acc[mf][nf][r];
      }
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, bool FAST>
__global__ __launch_bounds__(kBlock) void conv_dgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ w_t, T* __restrict__ dx,
    ConvShape sh) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MF = WM / CFRAG, NF = WN / CFRAG;
  __shared__ T a_lds[2][BM * lds_row_elems<T>()];
  __shared__ T b_lds[2][BN * lds_row_elems<T>()];
  const int Mtot = sh.N * sh.H * sh.W;
  const int Ntot = sh.Cin;
  const int Ktot = sh.KH * sh.KW * sh.Cout;
  // XCD-aware remap (see gemm.hip)
  int t_n, t_m;
  {
    const int nwg = gridDim.x * gridDim.y;
    int bid = blockIdx.y * gridDim.x + blockIdx.x;
    if (sh.swz && nwg >= 64) {
      const int q = nwg >> 3, r = nwg & 7;
      const int xcd = bid & 7, idx = bid >> 3;
      bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    t_n = bid % gridDim.x;
    t_m = bid / gridDim.x;
  }
  const int m0 = t_m * BM, n0 = t_n * BN;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
  f32x4 acc[MF][NF] = {};
  const int nk = (Ktot + CBK - 1) / CBK;
  DgradAStager<T, BM, FAST> sa;
  sa.init(sh, m0, Mtot);
  sa.stage(a_lds[0], dy, sh, Ktot);
  // B from the TRANSPOSED weight copy w_t [Cin][KH*KW*Cout] (row-major,
  // k-contiguous: same staging as forward B, glds-eligible)
  stage_fwd_B<T, BN>(b_lds[0], w_t, n0, 0, Ntot, Ktot, Ktot);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      sa.stage(a_lds[cur ^ 1], dy, sh, Ktot);
      stage_fwd_B<T, BN>(b_lds[cur ^ 1], w_t, n0, (kt + 1) * CBK, Ntot, Ktot, Ktot);
    }
    conv_mma<T, MF, NF>(a_lds[cur], b_lds[cur], acc, lane, wm0, wn0);
    __syncthreads();
  }
  const int col_in_frag = lane & 15, row_base = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm0 + mf * CFRAG + row_base + r;
        int col = n0 + wn0 + nf * CFRAG + col_in_frag;
        if (row < Mtot && col < Ntot)
          dx[(long long)row * Ntot + col] = (T)acc[mf][nf][r];
      }
}

// Stride-2 dgrad, phase-decomposed (dgrad_phase_map.h): an M tile holds
// input pixels of ONE parity class and the K loop walks only that class's
// taps x Cout — the k-steps the kernel above would stage as zero rows are
// never issued. The remaining k-steps are the same ones in the same order,
// so the result is bit-identical. Needs Cout % CBK == 0 (a k-step never
// spans two taps). 1-D grid: n tile fastest, classes heaviest first.
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(kBlock) void conv_dgrad_phase_kernel(
    const T* __restrict__ dy, const T* __restrict__ w_t, T* __restrict__ dx,
    ConvShape sh, dgph::Map mp) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MF = WM / CFRAG, NF = WN / CFRAG;
  static_assert(BM <= kBlock, "one thread per row fills row_px");
  __shared__ T a_lds[2][BM * lds_row_elems<T>()];
  __shared__ T b_lds[2][BN * lds_row_elems<T>()];
  __shared__ int row_px[BM];     // flat input pixel of a tile row, -1 past the class
  const int Ntot = sh.Cin;
  const int Ktot = sh.KH * sh.KW * sh.Cout;
  const int n_tiles = (Ntot + BN - 1) / BN;
  const dgph::Tile tile = dgph::block_tile(mp, blockIdx.x, n_tiles, sh.swz);
  const dgph::Class& cls = mp.cls[tile.cls];
  const int r0 = tile.m_tile * BM, n0 = tile.n_tile * BN;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
  f32x4 acc[MF][NF] = {};
  const int nk = cls.ntaps * (sh.Cout / CBK);   // 0 for a class without taps
  if (threadIdx.x < BM) {
    const int r = r0 + threadIdx.x;
    row_px[threadIdx.x] = r < cls.rows ? dgph::row_pixel(mp, cls, r) : -1;
  }
  DgradPhaseAStager<T, BM> sa;
  sa.init(cls, r0);
  int tap = cls.tap0, co0 = 0;                  // block-uniform k cursor
  auto stage = [&](int buf) {
    const dgph::Tap tp = mp.taps[tap];
    sa.stage(a_lds[buf], dy, sh, tp.dh, tp.dw, co0);
    stage_fwd_B<T, BN>(b_lds[buf], w_t, n0,
                       (tp.kh * sh.KW + tp.kw) * sh.Cout + co0, Ntot, Ktot, Ktot);
    co0 += CBK;
    if (co0 == sh.Cout) { co0 = 0; ++tap; }
  };
  if (nk > 0) stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(cur ^ 1);
    conv_mma<T, MF, NF>(a_lds[cur], b_lds[cur], acc, lane, wm0, wn0);
    __syncthreads();
  }
  const int col_in_frag = lane & 15, row_base = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int px = row_px[wm0 + mf * CFRAG + row_base + r];
      if (px < 0) continue;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int col = n0 + wn0 + nf * CFRAG + col_in_frag;
        if (col < Ntot) dx[(long long)px * Ntot + col] = (T)acc[mf][nf][r];
      }
    }
}

// Split-K over pixels (see launcher): partials -> fp32 atomics.
template <typename T, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(kBlock) void conv_wgrad_kernel(
    const T* __restrict__ dy_t, const T* __restrict__ x, float* __restrict__ dw,
    ConvShape sh, long long p_chunk) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int MF = WM / CFRAG, NF = WN / CFRAG;
  __shared__ T a_lds[2][BM * lds_row_elems<T>()];
  __shared__ T b_lds[2][BN * lds_row_elems<T>()];
  const int Mtot = sh.Cout;
  const int Ntot = sh.KH * sh.KW * sh.Cin;
  const long long Ptot = (long long)sh.N * sh.HO * sh.WO;
  const long long p_begin = (long long)blockIdx.z * p_chunk;
  const long long p_end = min(p_begin + p_chunk, Ptot);
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
  f32x4 acc[MF][NF] = {};
  const long long nk = (p_end - p_begin + CBK - 1) / CBK;
  if (nk <= 0) return;
  WgradBStager<T, BN> sb;
  sb.init(sh, n0, p_begin, p_end, Ntot);
  // A from the TRANSPOSED dy copy [Cout][P] (k = pixel contiguous): plain
  // direct staging (glds-eligible) instead of scalar transposed writes
  stage_fwd_B<T, BM>(a_lds[0], dy_t, m0, (int)p_begin, Mtot, (int)p_end, Ptot);
  sb.stage(b_lds[0], x, sh);
  __syncthreads();
  for (long long kt = 0; kt < nk; ++kt) {
    const int cur = (int)(kt & 1);
    if (kt + 1 < nk) {
      stage_fwd_B<T, BM>(a_lds[cur ^ 1], dy_t, m0,
                         (int)(p_begin + (kt + 1) * CBK), Mtot, (int)p_end,
                         Ptot);
      sb.set_p_ok(p_begin + (kt + 1) * CBK, p_end);
      sb.stage(b_lds[cur ^ 1], x, sh);
    }
    conv_mma<T, MF, NF>(a_lds[cur], b_lds[cur], acc, lane, wm0, wn0);
    __syncthreads();
  }
  const int col_in_frag = lane & 15, row_base = (lane >> 4) * 4;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = m0 + wm0 + mf * CFRAG + row_base + r;
        int col = n0 + wn0 + nf * CFRAG + col_in_frag;
        if (row < Mtot && col < Ntot) {
          if (gridDim.z == 1)
            dw[(long long)row * Ntot + col] = acc[mf][nf][r];
          else
            atomicAdd(&dw[(long long)row * Ntot + col], acc[mf][nf][r]);
        }
      }
}

// Instantiations: Big = 128x128 (2x2), NarrowN = 128x64 (4x1),
// NarrowM (wgrad) = 64x128 (1x4); FAST per channel divisibility.
#define INST_CONV(T)                                                        \
  template __global__ void conv_fwd_kernel<T, 128, 128, 2, 2, true>(        \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_fwd_kernel<T, 128, 128, 2, 2, false>(       \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_fwd_kernel<T, 128, 64, 4, 1, true>(         \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_fwd_kernel<T, 128, 64, 4, 1, false>(        \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_dgrad_kernel<T, 128, 128, 2, 2, true>(      \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_dgrad_kernel<T, 128, 128, 2, 2, false>(     \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_dgrad_kernel<T, 128, 64, 4, 1, true>(       \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_dgrad_kernel<T, 128, 64, 4, 1, false>(      \
      const T*, const T*, T*, ConvShape);                                   \
  template __global__ void conv_dgrad_phase_kernel<T, 128, 128, 2, 2>(      \
      const T*, const T*, T*, ConvShape, dgph::Map);                        \
  template __global__ void conv_dgrad_phase_kernel<T, 128, 64, 4, 1>(       \
      const T*, const T*, T*, ConvShape, dgph::Map);                        \
  template __global__ void conv_wgrad_kernel<T, 128, 128, 2, 2>(            \
      const T*, const T*, float*, ConvShape, long long);                    \
  template __global__ void conv_wgrad_kernel<T, 64, 128, 1, 4>(             \
      const T*, const T*, float*, ConvShape, long long);

INST_CONV(bf16)
INST_CONV(float)

// ---- launchers -------------------------------------------------------------
// conv_route.h decides; these launch what the route names and refuse a
// route of another kind or one that does not cover the problem.
#include "launchers.h"

static ConvShape make_shape(const ConvRoute& rt, const ConvProblem& p) {
  ConvShape sh;
  sh.N = p.N; sh.H = p.H; sh.W = p.W; sh.Cin = p.Cin; sh.Cout = p.Cout;
  sh.KH = p.KH; sh.KW = p.KW; sh.stride = p.stride; sh.pad = p.pad;
  sh.HO = rt.HO;
  sh.WO = rt.WO;
  sh.swz = rt.use_swz;
  return sh;
}

// HO / WO and the generic tile (128 pixels x 64 or 128 columns) are what
// the kernels derive their indexing from
static bool generic_tile_fits(const ConvRoute& rt, const ConvProblem& p) {
  return rt.HO == conv_out(p.H, p.KH, p.stride, p.pad) &&
         rt.WO == conv_out(p.W, p.KW, p.stride, p.pad) && rt.HO > 0 &&
         rt.WO > 0 && rt.bm == 128 && (rt.bn == 64 || rt.bn == 128);
}

bool launch_conv_fwd(const ConvRoute& rt, const ConvProblem& p, const void* x,
                     const void* w, void* y, hipStream_t s) {
  if (rt.kind != ConvKind::Generic || p.op != ConvOp::Fwd ||
      !generic_tile_fits(rt, p) || !conv_grid_fits(rt, p, rt.bm, rt.bn) ||
      (rt.fast && p.Cin % CBK != 0))
    return false;
  const ConvShape sh = make_shape(rt, p);
  const bool narrow = rt.bn == 64, fast = rt.fast;
  dim3 grid(rt.grid_x, rt.grid_y);
  #define FWD(T, BM, BN, WM, WN, F)                                         \
    hipLaunchKernelGGL((conv_fwd_kernel<T, BM, BN, WM, WN, F>), grid,       \
                       dim3(kBlock), 0, s, (const T*)x, (const T*)w, (T*)y, sh)
  if (p.bf16) {
    if (narrow) { if (fast) FWD(bf16, 128, 64, 4, 1, true); else FWD(bf16, 128, 64, 4, 1, false); }
    else { if (fast) FWD(bf16, 128, 128, 2, 2, true); else FWD(bf16, 128, 128, 2, 2, false); }
  } else {
    if (narrow) { if (fast) FWD(float, 128, 64, 4, 1, true); else FWD(float, 128, 64, 4, 1, false); }
    else { if (fast) FWD(float, 128, 128, 2, 2, true); else FWD(float, 128, 128, 2, 2, false); }
  }
  #undef FWD
  return true;
}

bool launch_conv_dgrad(const ConvRoute& rt, const ConvProblem& p,
                       const void* dy, const void* w, void* dx,
                       hipStream_t s) {
  if (p.op != ConvOp::Dgrad || !generic_tile_fits(rt, p)) return false;
  const ConvShape sh = make_shape(rt, p);
  const bool narrow = rt.bn == 64;
  // stride 2: phase-decomposed, only the live taps of each parity class
  if (rt.kind == ConvKind::DgradPhase) {
    if (!conv_dgrad_phase_fits(p)) return false;
    const dgph::Map mp = dgph::make_map(p.N, p.H, p.W, p.KH, p.KW, p.pad, 128);
    if (rt.grid_x != mp.m_tiles * ((p.Cin + rt.bn - 1) / rt.bn) ||
        rt.grid_y != 1 || rt.grid_z != 1)
      return false;
    dim3 pgrid((unsigned)rt.grid_x);
    #define DGP(T, BM, BN, WM, WN)                                          \
      hipLaunchKernelGGL((conv_dgrad_phase_kernel<T, BM, BN, WM, WN>),      \
                         pgrid, dim3(kBlock), 0, s, (const T*)dy,           \
                         (const T*)w, (T*)dx, sh, mp)
    if (p.bf16) { if (narrow) DGP(bf16, 128, 64, 4, 1); else DGP(bf16, 128, 128, 2, 2); }
    else { if (narrow) DGP(float, 128, 64, 4, 1); else DGP(float, 128, 128, 2, 2); }
    #undef DGP
    return true;
  }
  if (rt.kind != ConvKind::Generic || !conv_grid_fits(rt, p, rt.bm, rt.bn) ||
      (rt.fast && p.Cout % CBK != 0))
    return false;
  const bool fast = rt.fast;
  dim3 grid(rt.grid_x, rt.grid_y);
  #define DG(T, BM, BN, WM, WN, F)                                          \
    hipLaunchKernelGGL((conv_dgrad_kernel<T, BM, BN, WM, WN, F>), grid,     \
                       dim3(kBlock), 0, s, (const T*)dy, (const T*)w, (T*)dx, sh)
  if (p.bf16) {
    if (narrow) { if (fast) DG(bf16, 128, 64, 4, 1, true); else DG(bf16, 128, 64, 4, 1, false); }
    else { if (fast) DG(bf16, 128, 128, 2, 2, true); else DG(bf16, 128, 128, 2, 2, false); }
  } else {
    if (narrow) { if (fast) DG(float, 128, 64, 4, 1, true); else DG(float, 128, 64, 4, 1, false); }
    else { if (fast) DG(float, 128, 128, 2, 2, true); else DG(float, 128, 128, 2, 2, false); }
  }
  #undef DG
  return true;
}

bool launch_conv_wgrad(const ConvRoute& rt, const ConvProblem& p,
                       const void* dy, const void* x, void* dw,
                       hipStream_t s) {
  // dw is ALWAYS the fp32 accumulation buffer (bindings allocate zeroed).
  // The pixel slices must tile [0, P) in whole k-steps.
  const long long Ptot = (long long)p.N * rt.HO * rt.WO;
  if (rt.kind != ConvKind::WgradGeneric || p.op != ConvOp::Wgrad ||
      rt.HO != conv_out(p.H, p.KH, p.stride, p.pad) ||
      rt.WO != conv_out(p.W, p.KW, p.stride, p.pad) || Ptot <= 0 ||
      Ptot >= (1LL << 31) || (rt.bm != 64 && rt.bm != 128) || rt.bn != 128 ||
      rt.grid_x != (p.KH * p.KW * p.Cin + 127) / 128 ||
      rt.grid_y != (p.Cout + rt.bm - 1) / rt.bm || rt.splits < 1 ||
      rt.grid_z != rt.splits || rt.p_chunk < CBK || rt.p_chunk % CBK != 0 ||
      rt.splits * rt.p_chunk < Ptot || (rt.splits - 1) * rt.p_chunk >= Ptot)
    return false;
  const ConvShape sh = make_shape(rt, p);
  const bool narrow_m = rt.bm == 64;
  const long long p_chunk = rt.p_chunk;
  dim3 grid(rt.grid_x, rt.grid_y, rt.splits);
  #define WG(T, BM, BN, WM, WN)                                             \
    hipLaunchKernelGGL((conv_wgrad_kernel<T, BM, BN, WM, WN>), grid,        \
                       dim3(kBlock), 0, s, (const T*)dy, (const T*)x,       \
                       (float*)dw, sh, p_chunk)
  if (p.bf16) { if (narrow_m) WG(bf16, 64, 128, 1, 4); else WG(bf16, 128, 128, 2, 2); }
  else { if (narrow_m) WG(float, 64, 128, 1, 4); else WG(float, 128, 128, 2, 2); }
  #undef WG
  return true;
}

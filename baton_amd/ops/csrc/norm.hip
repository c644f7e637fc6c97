// Normalization kernels (gfx950): LayerNorm, RMSNorm and BatchNorm (NHWC),
// fwd + bwd. norm_route.h decides every grid and kernel form; the launchers
// at the end launch exactly what a route names.
//
// Not present in the reference (SURVEY.md §2.2 — its only model is
// Linear(10,1)) but required by the ResNet / BERT / Llama federated configs.
//
// LayerNorm / RMSNorm: one block per row, block-reduced statistics, saved
// (mean, rstd) for backward; dgamma / dbeta by a column-chunk reduction
// (coalesced in NHWC / row-major since consecutive lanes read consecutive
// channels). BatchNorm (training): per-channel stats by column-chunk
// reduction with a rows-split atomicAdd pass, then a vectorized normalize
// pass; eval mode normalizes with running stats.
#include "common.h"
#include "norm_route.h"

static_assert(kNormBlock == kBlock && kNormMaxGrid == kMaxGrid,
              "norm_route.h sizes its grids for common.h's block and cap");

// Row index of the row kernels: LayerNorm's rows fit int (bindings.cpp
// refuses more) and its kernels keep the int loop. Under the 64-bit loop that
// RMSNorm needs, LayerNorm's forward took up to 8 more VGPRs and the dx pass
// of ln_bwd_plus ran 1.5x as long (profiles/r06_norm_refactor.md).
template <bool MEAN>
using NormRow = std::conditional_t<MEAN, int, long long>;

// ---- LayerNorm / RMSNorm forward ---------------------------------------------
// MEAN (LayerNorm): y = (x - mu) rstd w + b, rstd = (var + eps)^-1/2 from the
// one-pass variance; saves (mean, rstd). Without MEAN (RMSNorm): y = x rstd w,
// rstd = (mean(x^2) + eps)^-1/2; saves rstd, b and mean_out are not touched.
// ADD fuses the transformer residual add (guide: fuse elementwise work into
// the producing pass): z = x + res is written ONCE here and the norm consumes
// it — the separate add kernel and one full tensor read disappear (the
// at::add glue in the r1 profiles, VERDICT weak #4).
template <typename T, bool MEAN, bool ADD>
__global__ void norm_fwd_kernel(const T* __restrict__ x,
                                const T* __restrict__ res,
                                const T* __restrict__ w, const T* __restrict__ b,
                                T* __restrict__ y, T* __restrict__ zout,
                                float* __restrict__ mean_out,
                                float* __restrict__ rstd_out, long long R, int C,
                                float eps) {
  __shared__ float scratch[kBlock / kWave];
  using Row = NormRow<MEAN>;
  for (Row r = blockIdx.x; r < (Row)R; r += gridDim.x) {
    const long long base = (long long)r * C;
    const T* row = x + base;
    T* yrow = y + base;
    float s = 0.f, ss = 0.f;
    row_walk<T>(C, [&](int c, auto width) {
      constexpr int W = decltype(width)::value;
      float f[W];
      vload<W>(row + c, f);
      if constexpr (ADD) {
        float fr[W];
        vload<W>(res + base + c, fr);
#pragma unroll
        for (int q = 0; q < W; ++q) f[q] += fr[q];
        vstore<W>(zout + base + c, f);
      }
#pragma unroll
      for (int q = 0; q < W; ++q) {
        if constexpr (MEAN) s += f[q];
        ss = fmaf(f[q], f[q], ss);
      }
    });
    float mu = 0.f, rstd;
    if constexpr (MEAN) {
      float sum = block_reduce_sum(s, scratch);
      float sumsq = block_reduce_sum(ss, scratch);
      mu = sum / C;
      float var = sumsq / C - mu * mu;
      rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    } else {
      float sumsq = block_reduce_sum(ss, scratch);
      rstd = rsqrtf(sumsq / C + eps);
    }
    if (threadIdx.x == 0) {
      if constexpr (MEAN) mean_out[r] = mu;
      rstd_out[r] = rstd;
    }
    // normalize pass re-reads the summed row (same CU wrote it; the
    // inter-CU L1 staleness hazard does not apply to a block's own lines)
    const T* zrow = ADD ? zout + base : row;
    row_walk<T>(C, [&](int c, auto width) {
      constexpr int W = decltype(width)::value;
      float f[W], fw[W];
      vload<W>(zrow + c, f);
      vload<W>(w + c, fw);
      if constexpr (MEAN) {
        float fb[W];
        vload<W>(b + c, fb);
#pragma unroll
        for (int q = 0; q < W; ++q)
          f[q] = fmaf((f[q] - mu) * rstd, fw[q], fb[q]);
      } else {
#pragma unroll
        for (int q = 0; q < W; ++q) f[q] = f[q] * rstd * fw[q];
      }
      vstore<W>(yrow + c, f);
    });
  }
}

// ---- LayerNorm / RMSNorm backward (dx) ----------------------------------------
// dyg = dy*w, xhat = (x - mu) rstd (mu = 0 without MEAN);
// MEAN:  dx = rstd * (dyg - mean(dyg) - xhat * mean(dyg*xhat))
// else:  dx = rstd * (dyg - xhat * mean(dyg*xhat))
// PLUS fuses the residual-stream gradient add (backward of the fused
// z = x + res forward): dx += plus, saving the separate add pass.
template <typename T, bool MEAN, bool PLUS>
__global__ void norm_bwd_dx_kernel(const T* __restrict__ x,
                                   const T* __restrict__ dy,
                                   const T* __restrict__ w,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const T* __restrict__ plus,
                                   T* __restrict__ dx, long long R, int C) {
  __shared__ float scratch[kBlock / kWave];
  using Row = NormRow<MEAN>;
  for (Row r = blockIdx.x; r < (Row)R; r += gridDim.x) {
    const long long base = (long long)r * C;
    const T* xrow = x + base;
    const T* dyrow = dy + base;
    T* dxrow = dx + base;
    const float rs = rstd[r];
    float mu = 0.f;
    if constexpr (MEAN) mu = mean[r];
    auto hat = [&](float v) {
      if constexpr (MEAN) return (v - mu) * rs;
      else return v * rs;
    };
    float s1 = 0.f, s2 = 0.f;
    row_walk<T>(C, [&](int c, auto width) {
      constexpr int W = decltype(width)::value;
      float fx[W], fd[W], fw[W];
      vload<W>(xrow + c, fx);
      vload<W>(dyrow + c, fd);
      vload<W>(w + c, fw);
#pragma unroll
      for (int q = 0; q < W; ++q) {
        float dyg = fd[q] * fw[q];
        if constexpr (MEAN) s1 += dyg;
        s2 = fmaf(dyg, hat(fx[q]), s2);
      }
    });
    float m1 = 0.f;
    if constexpr (MEAN) m1 = block_reduce_sum(s1, scratch) / C;
    float m2 = block_reduce_sum(s2, scratch) / C;
    row_walk<T>(C, [&](int c, auto width) {
      constexpr int W = decltype(width)::value;
      float fx[W], fd[W], fw[W];
      vload<W>(xrow + c, fx);
      vload<W>(dyrow + c, fd);
      vload<W>(w + c, fw);
#pragma unroll
      for (int q = 0; q < W; ++q) {
        float dyg = fd[q] * fw[q];
        float xhat = hat(fx[q]);
        if constexpr (MEAN) fd[q] = rs * (dyg - m1 - xhat * m2);
        else fd[q] = rs * (dyg - xhat * m2);
      }
      if constexpr (PLUS) {
        float fp[W];
        vload<W>(plus + base + c, fp);
#pragma unroll
        for (int q = 0; q < W; ++q) fd[q] += fp[q];
      }
      vstore<W>(dxrow + c, fd);
    });
  }
}

// ---- column reductions -------------------------------------------------------
// N per-channel sums over rows with BOTH channel and row parallelism: a block
// covers 64 channels x 4 row lanes (all 256 threads busy even at C = 64),
// rows additionally split over grid.y. term(r, c, acc) adds row r of channel
// c to acc[0..N); the 4 lane partials combine in LDS, then one atomicAdd per
// channel into out[i] (zero-initialized by the caller) or, with DIRECT and a
// single row block, a plain store. The previous one-thread-per-channel form
// left ~3 blocks running on 256 CUs and was 49% of the BERT step.
template <int N, bool DIRECT, typename F>
DEVINL void col_reduce_4x64(long long R, int C, int rows_per_block,
                            float* const (&out)[N], F&& term) {
  __shared__ float part[N][4][64];
  const int c_local = threadIdx.x & 63;
  const int row_lane = threadIdx.x >> 6;         // 0..3
  const int c = blockIdx.x * 64 + c_local;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  const long long r1 = min(r0 + rows_per_block, R);
  float acc[N] = {};
  if (c < C) {
    for (long long r = r0 + row_lane; r < r1; r += 4) term(r, c, acc);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) part[i][row_lane][c_local] = acc[i];
  __syncthreads();
  if (row_lane == 0 && c < C) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float t = part[i][0][c_local] + part[i][1][c_local] +
                part[i][2][c_local] + part[i][3][c_local];
      if (DIRECT && gridDim.y == 1) out[i][c] = t;
      else atomicAdd(&out[i][c], t);
    }
  }
}

// Vector form (C % 64 == 0, the ResNet case): each thread owns an 8-channel
// run read as 16-B vectors (G13 — the 4 x 64 walk issues 2-B loads) and 32
// row lanes stream rows r_begin, r_begin + 32, ... < r_end. The kernel walks
// its rows into two 8-wide sums and puts them into row `lane` of its two
// padded LDS tiles (from its own registers: handing the arrays to a helper
// makes the compiler keep them as one vector and scalarize the packed
// subtractions); col32x8_finish column-reduces the tiles with 64 threads,
// then atomics. ~1.5x the 4 x 64 form at bench shapes.
using Col32x8Tile = float[32][65];   // +1 pad: column reduce reads

struct Col32x8 {
  int lane, col;              // tile row (0..31) and first tile column (0..56)
  int ch;                     // first of this thread's 8 channels
  long long r_begin, r_end;
};

DEVINL Col32x8 col32x8_begin(long long M, int rows_per_block) {
  const int c8 = threadIdx.x & 7;
  const int rl = threadIdx.x >> 3;
  const long long r0 = (long long)blockIdx.y * rows_per_block;
  return {rl, c8 * 8, (int)(blockIdx.x * 64 + c8 * 8), r0 + rl,
          min(r0 + rows_per_block, M)};
}

DEVINL void col32x8_finish(Col32x8Tile& l1, Col32x8Tile& l2,
                           float* __restrict__ out1, float* __restrict__ out2) {
  __syncthreads();
  if (threadIdx.x < 64) {
    float t1 = 0.f, t2 = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      t1 += l1[r][threadIdx.x];
      t2 += l2[r][threadIdx.x];
    }
    atomicAdd(&out1[blockIdx.x * 64 + threadIdx.x], t1);
    atomicAdd(&out2[blockIdx.x * 64 + threadIdx.x], t2);
  }
}

// dw[c] = sum_r dy*xhat; with MEAN (LayerNorm) also db[c] = sum_r dy.
template <typename T, bool MEAN>
__global__ void norm_bwd_dw_kernel(const T* __restrict__ x,
                                   const T* __restrict__ dy,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   float* __restrict__ dw,
                                   float* __restrict__ db, long long R, int C,
                                   int rows_per_block) {
  if constexpr (MEAN) {
    float* const out[2] = {dw, db};
    col_reduce_4x64<2, true>(
        R, C, rows_per_block, out, [&](long long r, int c, float* acc) {
          float d = (float)dy[r * C + c];
          float xhat = ((float)x[r * C + c] - mean[r]) * rstd[r];
          acc[0] = fmaf(d, xhat, acc[0]);
          acc[1] += d;
        });
  } else {
    float* const out[1] = {dw};
    col_reduce_4x64<1, true>(
        R, C, rows_per_block, out, [&](long long r, int c, float* acc) {
          acc[0] = fmaf((float)dy[r * C + c], (float)x[r * C + c] * rstd[r],
                        acc[0]);
        });
  }
}

// ---- BatchNorm (NHWC: input viewed as [M rows, C channels]) ----------------

// Pass 1: per-channel sum & sumsq. Blocks tile (channel chunk, row chunk);
// row chunks atomically accumulate into sum[c]/sumsq[c] (caller zeroes).
template <typename T>
__global__ void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ sum,
                                float* __restrict__ sumsq, long long M, int C,
                                int rows_per_block) {
  float* const out[2] = {sum, sumsq};
  col_reduce_4x64<2, false>(M, C, rows_per_block, out,
                            [&](long long r, int c, float* acc) {
                              float v = (float)x[r * C + c];
                              acc[0] += v;
                              acc[1] = fmaf(v, v, acc[1]);
                            });
}

template <typename T>
__global__ void bn_stats_vec_kernel(const T* __restrict__ x,
                                    float* __restrict__ sum,
                                    float* __restrict__ sumsq, long long M,
                                    int C, int rows_per_block) {
  constexpr int V = VecTraits<T>::kElems;
  __shared__ Col32x8Tile l1, l2;
  const Col32x8 t = col32x8_begin(M, rows_per_block);
  float s[8] = {}, ss[8] = {};
  // fp32 (V == 4): the run is two vectors, each walked over the rows in turn
#pragma unroll
  for (int part = 0; part < 8 / V; ++part) {
    for (long long r = t.r_begin; r < t.r_end; r += 32) {
      float f[V];
      vload16(&x[r * C + t.ch + part * V], f);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        s[part * V + q] += f[q];
        ss[part * V + q] = fmaf(f[q], f[q], ss[part * V + q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    l1[t.lane][t.col + q] = s[q];
    l2[t.lane][t.col + q] = ss[q];
  }
  col32x8_finish(l1, l2, sum, sumsq);
}

// Backward pass 1: per-channel sum(dy) and sum(dy*xhat). With RELU, dy is
// masked by (y > 0) first (y = the post-ReLU output, also masked in dx).
template <typename T, bool RELU>
__global__ void bn_bwd_stats_kernel(const T* __restrict__ x,
                                    const T* __restrict__ dy,
                                    const T* __restrict__ y_post,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    float* __restrict__ sum_dy,
                                    float* __restrict__ sum_dyx, long long M,
                                    int C, int rows_per_block) {
  float* const out[2] = {sum_dy, sum_dyx};
  col_reduce_4x64<2, false>(
      M, C, rows_per_block, out, [&](long long r, int c, float* acc) {
        const float mu = mean[c], rs = rstd[c];   // loop-invariant: hoisted
        float d = (float)dy[r * C + c];
        if (RELU) d = ((float)y_post[r * C + c] > 0.f) ? d : 0.f;
        float xhat = ((float)x[r * C + c] - mu) * rs;
        acc[0] += d;
        acc[1] = fmaf(d, xhat, acc[1]);
      });
}

template <typename T, bool RELU>
__global__ void bn_bwd_stats_vec_kernel(
    const T* __restrict__ x, const T* __restrict__ dy,
    const T* __restrict__ y_post, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ sum_dy,
    float* __restrict__ sum_dyx, long long M, int C, int rows_per_block) {
  using VT = VecTraits<T>;
  constexpr int V = VT::kElems;
  __shared__ Col32x8Tile l1, l2;
  const Col32x8 t = col32x8_begin(M, rows_per_block);
  float mu[8], rs[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    mu[q] = mean[t.ch + q];
    rs[q] = rstd[t.ch + q];
  }
  float s1v[8] = {}, s2v[8] = {};
  for (long long r = t.r_begin; r < t.r_end; r += 32) {
#pragma unroll
    for (int part = 0; part < 8 / V; ++part) {
      const long long base = r * C + t.ch + part * V;
      float fx[V], fd[V], fy[V];
      typename VT::VecT vx =
          *reinterpret_cast<const typename VT::VecT*>(&x[base]);
      typename VT::VecT vd =
          *reinterpret_cast<const typename VT::VecT*>(&dy[base]);
      VT::to_float(vx, fx);
      VT::to_float(vd, fd);
      if (RELU) {
        typename VT::VecT vy =
            *reinterpret_cast<const typename VT::VecT*>(&y_post[base]);
        VT::to_float(vy, fy);
      }
#pragma unroll
      for (int q = 0; q < V; ++q) {
        float d = fd[q];
        if (RELU) d = fy[q] > 0.f ? d : 0.f;
        const int qq = part * V + q;
        float xhat = (fx[q] - mu[qq]) * rs[qq];
        s1v[qq] += d;
        s2v[qq] = fmaf(d, xhat, s2v[qq]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    l1[t.lane][t.col + q] = s1v[q];
    l2[t.lane][t.col + q] = s2v[q];
  }
  col32x8_finish(l1, l2, sum_dy, sum_dyx);
}

// Pass 2 (one small block over C): finalize mean/rstd, update running stats.
__global__ void bn_finalize_kernel(const float* __restrict__ sum,
                                   const float* __restrict__ sumsq,
                                   float* __restrict__ mean,
                                   float* __restrict__ rstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var, long long M,
                                   int C, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float mu = sum[c] / (float)M;
  float var = sumsq[c] / (float)M - mu * mu;  // biased (torch normalizes with biased)
  var = fmaxf(var, 0.f);
  mean[c] = mu;
  rstd[c] = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    float unbiased = M > 1 ? var * (float)M / (float)(M - 1) : var;
    running_mean[c] = fmaf(momentum, mu - running_mean[c], running_mean[c]);
    running_var[c] = fmaf(momentum, unbiased - running_var[c], running_var[c]);
  }
}

// Pass 3: y = (x - mean) * rstd * gamma + beta, optional fused ReLU;
// ADDIN fuses the ResNet residual join (y = relu(bn(x) + res)) — the
// standalone add_relu pass and one full activation read disappear.
template <typename T, bool RELU, bool ADDIN = false>
__global__ void bn_norm_kernel(const T* __restrict__ x,
                               const T* __restrict__ res,
                               const float* __restrict__ mean,
                               const float* __restrict__ rstd,
                               const float* __restrict__ gamma,
                               const float* __restrict__ beta,
                               T* __restrict__ y, long long M, int C) {
  const long long total = M * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    float v = ((float)x[i] - mean[c]) * rstd[c];
    v = fmaf(v, gamma[c], beta[c]);
    if (ADDIN) v += (float)res[i];
    if (RELU) v = fmaxf(v, 0.f);
    y[i] = (T)v;
  }
}

// Vectorized normalize (C % kElems == 0): y = x*K1[c] + K2[c] — the two
// per-channel constants are precomputed into LDS once per block, then the
// main loop is pure 16-B traffic (the scalar form costs a %C and four
// scalar param loads per ELEMENT).
template <typename T, bool RELU, bool ADDIN = false>
__global__ void bn_norm_vec_kernel(const T* __restrict__ x,
                                   const T* __restrict__ res,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   T* __restrict__ y, long long M, int C) {
  using VT = VecTraits<T>;
  constexpr int V = VT::kElems;
  extern __shared__ float bn_sm[];
  float* K1 = bn_sm;          // rstd*gamma
  float* K2 = bn_sm + C;      // beta - mean*rstd*gamma
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float g = rstd[c] * gamma[c];
    K1[c] = g;
    K2[c] = fmaf(-mean[c], g, beta[c]);
  }
  __syncthreads();
  const long long nvec = M * C / V;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)((i * V) % C);
    typename VT::VecT v = reinterpret_cast<const typename VT::VecT*>(x)[i];
    float f[V];
    VT::to_float(v, f);
    float fr[V];
    if (ADDIN) {
      typename VT::VecT vr = reinterpret_cast<const typename VT::VecT*>(res)[i];
      VT::to_float(vr, fr);
    }
#pragma unroll
    for (int q = 0; q < V; ++q) {
      f[q] = fmaf(f[q], K1[c0 + q], K2[c0 + q]);
      if (ADDIN) f[q] += fr[q];
      if (RELU) f[q] = fmaxf(f[q], 0.f);
    }
    typename VT::VecT o;
    VT::from_float(f, o);
    reinterpret_cast<typename VT::VecT*>(y)[i] = o;
  }
}

// Vectorized dx: dx = K1[c]*d - x*K3[c] + K4[c] (d optionally ReLU-masked
// by y_post), constants folded per channel in LDS.
// DRES additionally writes the residual-branch gradient of the fused
// y = relu(bn(x) + res) forward: dres = relu-masked dy (same mask as dx's).
template <typename T, bool RELU, bool DRES = false>
__global__ void bn_bwd_dx_vec_kernel(
    const T* __restrict__ x, const T* __restrict__ dy,
    const T* __restrict__ y_post, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ sum_dy, const float* __restrict__ sum_dyx,
    T* __restrict__ dx, T* __restrict__ dres, long long M, int C) {
  using VT = VecTraits<T>;
  constexpr int V = VT::kElems;
  extern __shared__ float bn_sm[];
  float* K1 = bn_sm;           // rstd*gamma
  float* K3 = bn_sm + C;       // rstd*gamma * rstd * sum_dyx/M
  float* K4 = bn_sm + 2 * C;   // mean*K3 - K1*sum_dy/M
  const float invM = 1.f / (float)M;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float g = rstd[c] * gamma[c];
    const float k3 = g * rstd[c] * sum_dyx[c] * invM;
    K1[c] = g;
    K3[c] = k3;
    K4[c] = fmaf(mean[c], k3, -g * sum_dy[c] * invM);
  }
  __syncthreads();
  const long long nvec = M * C / V;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)((i * V) % C);
    float fx[V], fd[V], fy[V];
    typename VT::VecT vx = reinterpret_cast<const typename VT::VecT*>(x)[i];
    typename VT::VecT vd = reinterpret_cast<const typename VT::VecT*>(dy)[i];
    VT::to_float(vx, fx);
    VT::to_float(vd, fd);
    if (RELU) {
      typename VT::VecT vy =
          reinterpret_cast<const typename VT::VecT*>(y_post)[i];
      VT::to_float(vy, fy);
    }
    float fdr[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      float d = fd[q];
      if (RELU) d = fy[q] > 0.f ? d : 0.f;
      if (DRES) fdr[q] = d;
      fd[q] = fmaf(d, K1[c0 + q], fmaf(-fx[q], K3[c0 + q], K4[c0 + q]));
    }
    typename VT::VecT o;
    VT::from_float(fd, o);
    reinterpret_cast<typename VT::VecT*>(dx)[i] = o;
    if (DRES) {
      typename VT::VecT orr;
      VT::from_float(fdr, orr);
      reinterpret_cast<typename VT::VecT*>(dres)[i] = orr;
    }
  }
}

// Backward pass 2: dx = rstd*gamma*(dy - sum_dy/M - xhat*sum_dyx/M)
template <typename T, bool RELU>
__global__ void bn_bwd_dx_kernel(const T* __restrict__ x,
                                 const T* __restrict__ dy,
                                 const T* __restrict__ y_post,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ sum_dy,
                                 const float* __restrict__ sum_dyx,
                                 T* __restrict__ dx, long long M, int C) {
  const long long total = M * C;
  const float invM = 1.f / (float)M;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    float d = (float)dy[i];
    if (RELU) d = ((float)y_post[i] > 0.f) ? d : 0.f;
    float xhat = ((float)x[i] - mean[c]) * rstd[c];
    float g = rstd[c] * gamma[c];
    dx[i] = (T)(g * (d - sum_dy[c] * invM - xhat * sum_dyx[c] * invM));
  }
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

// dtype x mode dispatch: calls f(TypeTag<T>, integral_constant<int, mode>)
// for T = bf16 / float and mode in [0, N), so each launcher names its kernel
// once and only the listed modes are instantiated (TypeTag: common.h).
template <typename T, int N, typename F>
static void dispatch_mode(int mode, F&& f) {
  if constexpr (N > 0) {
    if (mode == N - 1) f(TypeTag<T>{}, std::integral_constant<int, N - 1>{});
    else dispatch_mode<T, N - 1>(mode, f);
  }
}

template <int N, typename F>
static void norm_dispatch(bool is_bf16, int mode, F&& f) {
  if (is_bf16) dispatch_mode<bf16, N>(mode, f);
  else dispatch_mode<float, N>(mode, f);
}

// mode bit 1 = MEAN (LayerNorm), bit 0 = ADD / PLUS
void launch_norm_fwd(const NormRowRoute& rt, bool is_bf16, bool center,
                     const void* x, const void* res, const void* w,
                     const void* b, void* y, void* zout, float* mean,
                     float* rstd, long long R, int C, float eps,
                     hipStream_t s) {
  norm_dispatch<4>(is_bf16, (center ? 2 : 0) + (res ? 1 : 0), [&](auto t, auto m) {
    using T = typename decltype(t)::type;
    constexpr int mode = decltype(m)::value;
    hipLaunchKernelGGL((norm_fwd_kernel<T, (mode & 2) != 0, (mode & 1) != 0>),
                       dim3(rt.grid), dim3(kBlock), 0, s, (const T*)x,
                       (const T*)res, (const T*)w, (const T*)b, (T*)y, (T*)zout,
                       mean, rstd, R, C, eps);
  });
}

void launch_norm_bwd(const NormRowRoute& rt, bool is_bf16, bool center,
                     const void* x, const void* dy, const void* w,
                     const float* mean, const float* rstd, const void* plus,
                     void* dx, float* dw, float* db, long long R, int C,
                     hipStream_t s) {
  norm_dispatch<4>(is_bf16, (center ? 2 : 0) + (plus ? 1 : 0), [&](auto t, auto m) {
    using T = typename decltype(t)::type;
    constexpr int mode = decltype(m)::value;
    constexpr bool MEAN = (mode & 2) != 0;
    hipLaunchKernelGGL((norm_bwd_dx_kernel<T, MEAN, (mode & 1) != 0>),
                       dim3(rt.grid), dim3(kBlock), 0, s, (const T*)x,
                       (const T*)dy, (const T*)w, mean, rstd, (const T*)plus,
                       (T*)dx, R, C);
    hipLaunchKernelGGL((norm_bwd_dw_kernel<T, MEAN>),
                       dim3(rt.chunks, rt.grid_y), dim3(kBlock), 0, s,
                       (const T*)x, (const T*)dy, mean, rstd, dw, db, R, C,
                       rt.rows_per_block);
  });
}

void launch_bn_stats(const BnRoute& rt, bool is_bf16, const void* x, float* sum,
                     float* sumsq, long long M, int C, hipStream_t s) {
  const dim3 grid(rt.chunks, rt.grid_y);
  norm_dispatch<1>(is_bf16, 0, [&](auto t, auto) {
    using T = typename decltype(t)::type;
    if (rt.stats_vec)   // 16-B path (every ResNet BN width)
      hipLaunchKernelGGL(bn_stats_vec_kernel<T>, grid, dim3(kBlock), 0, s,
                         (const T*)x, sum, sumsq, M, C, rt.rows_per_block);
    else
      hipLaunchKernelGGL(bn_stats_kernel<T>, grid, dim3(kBlock), 0, s,
                         (const T*)x, sum, sumsq, M, C, rt.rows_per_block);
  });
}

void launch_bn_finalize(const float* sum, const float* sumsq, float* mean,
                        float* rstd, float* running_mean, float* running_var,
                        long long M, int C, float eps, float momentum,
                        hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, s, sum, sumsq, mean, rstd, running_mean,
                     running_var, M, C, eps, momentum);
}

// mode 0 plain, 1 fused ReLU, 2 fused residual add + ReLU
void launch_bn_norm(const BnRoute& rt, bool is_bf16, bool relu, const void* x,
                    const void* res, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, void* y, long long M,
                    int C, hipStream_t s) {
  norm_dispatch<3>(is_bf16, res ? 2 : relu ? 1 : 0, [&](auto t, auto m) {
    using T = typename decltype(t)::type;
    constexpr bool RELU = decltype(m)::value >= 1, ADDIN = decltype(m)::value == 2;
    if (rt.norm_vec)   // 16-B vectors + LDS constants
      hipLaunchKernelGGL((bn_norm_vec_kernel<T, RELU, ADDIN>),
                         dim3(rt.elem_grid), dim3(kBlock), rt.norm_lds, s,
                         (const T*)x, (const T*)res, mean, rstd, gamma, beta,
                         (T*)y, M, C);
    else
      hipLaunchKernelGGL((bn_norm_kernel<T, RELU, ADDIN>), dim3(rt.elem_grid),
                         dim3(kBlock), 0, s, (const T*)x, (const T*)res, mean,
                         rstd, gamma, beta, (T*)y, M, C);
  });
}

void launch_bn_bwd_stats(const BnRoute& rt, bool is_bf16, bool relu,
                         const void* x, const void* dy, const void* y_post,
                         const float* mean, const float* rstd, float* sum_dy,
                         float* sum_dyx, long long M, int C, hipStream_t s) {
  const dim3 grid(rt.chunks, rt.grid_y);
  norm_dispatch<2>(is_bf16, relu ? 1 : 0, [&](auto t, auto m) {
    using T = typename decltype(t)::type;
    constexpr bool RELU = decltype(m)::value == 1;
    if (rt.stats_vec)
      hipLaunchKernelGGL((bn_bwd_stats_vec_kernel<T, RELU>), grid, dim3(kBlock),
                         0, s, (const T*)x, (const T*)dy, (const T*)y_post,
                         mean, rstd, sum_dy, sum_dyx, M, C, rt.rows_per_block);
    else
      hipLaunchKernelGGL((bn_bwd_stats_kernel<T, RELU>), grid, dim3(kBlock), 0,
                         s, (const T*)x, (const T*)dy, (const T*)y_post, mean,
                         rstd, sum_dy, sum_dyx, M, C, rt.rows_per_block);
  });
}

// mode 0 plain, 1 ReLU-masked, 2 ReLU-masked + dres (vector pass only:
// rt.dres_ok, which bindings.cpp refuses without)
void launch_bn_bwd_dx(const BnRoute& rt, bool is_bf16, bool relu, const void* x,
                      const void* dy, const void* y_post, const float* mean,
                      const float* rstd, const float* gamma,
                      const float* sum_dy, const float* sum_dyx, void* dx,
                      void* dres, long long M, int C, hipStream_t s) {
  norm_dispatch<3>(is_bf16, dres ? 2 : relu ? 1 : 0, [&](auto t, auto m) {
    using T = typename decltype(t)::type;
    constexpr bool RELU = decltype(m)::value >= 1, DRES = decltype(m)::value == 2;
    if (rt.dx_vec)   // 16-B vectors + LDS constants
      hipLaunchKernelGGL((bn_bwd_dx_vec_kernel<T, RELU, DRES>),
                         dim3(rt.elem_grid), dim3(kBlock), rt.dx_lds, s,
                         (const T*)x, (const T*)dy, (const T*)y_post, mean, rstd,
                         gamma, sum_dy, sum_dyx, (T*)dx, (T*)dres, M, C);
    else
      hipLaunchKernelGGL((bn_bwd_dx_kernel<T, RELU>), dim3(rt.elem_grid),
                         dim3(kBlock), 0, s, (const T*)x, (const T*)dy,
                         (const T*)y_post, mean, rstd, gamma, sum_dy, sum_dyx,
                         (T*)dx, M, C);
  });
}

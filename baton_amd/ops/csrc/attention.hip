// Attention softmax kernels (gfx950).
//
// The transformer configs (BERT-base MLM, Llama-LoRA — BASELINE.json 3/4)
// compute attention as batched MFMA GEMMs (gemm.hip, grid.z = B*H) around
// this row softmax: y = softmax(scale * x [+ causal mask]) over the last
// dim. One block per row, online two-pass (max, then exp-sum), fused scale
// and causal masking — the score matrix is read once and written once.
// Backward fuses the dsoftmax reduction: dx = scale * y * (dy - sum(dy*y)).
#include "common.h"
#include "attn_route.h"

static_assert(kSoftmaxMaxGrid == kMaxGrid, "attn_route.h names this cap");

// Per-sequence key lengths (right padding). The VARLEN instantiations take a
// RowLens as their last argument: row r belongs to entry r / rows_per_len of
// kv_len and has query position r % q_period. Its columns stop at
// min(causal limit, L) with L = clamp(kv_len[entry], 0, C); a row whose query
// position is >= L is stored as zeros without being read. The dense
// instantiations take an empty struct and keep their code.
struct RowLens {
  const int* kv_len;
  long long rows_per_len;
  int q_period;
};
template <bool VARLEN> using Lens = LenArg<VARLEN, RowLens>;

// last visible column of row r given its dense limit qpos; -1: a dead row
DEVINL int len_limit(const RowLens& lens, long long r, int C, int qpos) {
  const int L = clamp_len(lens.kv_len[r / lens.rows_per_len], C);
  return (int)(r % lens.q_period) >= L ? -1 : min(qpos, L - 1);
}

template <typename T, bool CAUSAL, bool VARLEN>
__global__ void softmax_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   long long R, int C, float scale,
                                   int causal_seq,
                                   Lens<VARLEN> lens) {
  __shared__ float scratch[kBlock / kWave];
  __shared__ float s_max;
  for (long long r = blockIdx.x; r < R; r += gridDim.x) {
    const T* row = x + r * C;
    T* yrow = y + r * C;
    int qpos = CAUSAL ? (int)(r % causal_seq) : C - 1;
    constexpr int V = VecTraits<T>::kElems;
    const bool vec = softmax_vec(C, V);   // attn_route.h
    if constexpr (VARLEN) {
      qpos = len_limit(lens, r, C, qpos);
      if (qpos < 0) {   // block-uniform: the whole block skips the barriers
        if (vec) {
          float f[V] = {};
          for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x)
            vstore16(yrow + cv * V, f);
        } else {
          for (int c = threadIdx.x; c < C; c += blockDim.x) yrow[c] = (T)0.f;
        }
        continue;
      }
    }
    float m = -INFINITY;
    if (vec) {
      for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (cv * V + q <= qpos) m = fmaxf(m, f[q] * scale);
      }
    } else {
      for (int c = threadIdx.x; c <= qpos; c += blockDim.x)
        m = fmaxf(m, (float)row[c] * scale);
    }
    {
      const int lane = threadIdx.x & (kWave - 1);
      const int wid = threadIdx.x / kWave;
      float wm = wave_reduce_max(m);
      if (lane == 0) scratch[wid] = wm;
      __syncthreads();
      if (threadIdx.x == 0) {
        float t = -INFINITY;
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i)
          t = fmaxf(t, scratch[i]);
        s_max = t;
      }
      __syncthreads();
    }
    const float m_all = s_max;
    float acc = 0.f;
    if (vec) {
      for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (cv * V + q <= qpos) acc += __expf(f[q] * scale - m_all);
      }
    } else {
      for (int c = threadIdx.x; c <= qpos; c += blockDim.x)
        acc += __expf((float)row[c] * scale - m_all);
    }
    float denom = block_reduce_sum(acc, scratch);
    const float inv = 1.f / denom;
    if (vec) {
      for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          f[q] = cv * V + q <= qpos ? __expf(f[q] * scale - m_all) * inv : 0.f;
        vstore16(yrow + cv * V, f);
      }
    } else {
      for (int c = threadIdx.x; c < C; c += blockDim.x)
        yrow[c] = (T)(c <= qpos ? __expf((float)row[c] * scale - m_all) * inv
                                : 0.f);
    }
    __syncthreads();
  }
}

// dx = scale * y * (dy - sum_c dy*y). Masked (y==0) columns get dx = 0.
template <typename T>
__global__ void softmax_bwd_kernel(const T* __restrict__ y,
                                   const T* __restrict__ dy, T* __restrict__ dx,
                                   long long R, int C, float scale) {
  __shared__ float scratch[kBlock / kWave];
  for (long long r = blockIdx.x; r < R; r += gridDim.x) {
    const T* yrow = y + r * C;
    const T* dyrow = dy + r * C;
    T* dxrow = dx + r * C;
    constexpr int V = VecTraits<T>::kElems;
    const bool vec = softmax_vec(C, V);
    float acc = 0.f;
    if (vec) {
      for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x) {
        float fy[V], fd[V];
        vload16(yrow + cv * V, fy);
        vload16(dyrow + cv * V, fd);
#pragma unroll
        for (int q = 0; q < V; ++q) acc = fmaf(fd[q], fy[q], acc);
      }
    } else {
      for (int c = threadIdx.x; c < C; c += blockDim.x)
        acc = fmaf((float)dyrow[c], (float)yrow[c], acc);
    }
    float dot = block_reduce_sum(acc, scratch);
    if (vec) {
      for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x) {
        float fy[V], fd[V];
        vload16(yrow + cv * V, fy);
        vload16(dyrow + cv * V, fd);
#pragma unroll
        for (int q = 0; q < V; ++q) fd[q] = scale * fy[q] * (fd[q] - dot);
        vstore16(dxrow + cv * V, fd);
      }
    } else {
      for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float yv = (float)yrow[c];
        dxrow[c] = (T)(scale * yv * ((float)dyrow[c] - dot));
      }
    }
    __syncthreads();
  }
}

// Wave-per-row softmax for short rows (C <= 1024): four independent
// waves per block, wave-shuffle reductions, no block barriers — the
// row-per-block form leaves most of a 256-thread block idle at S=128.
template <typename T, bool CAUSAL, bool VARLEN>
__global__ __launch_bounds__(kBlock) void softmax_fwd_wave_kernel(
    const T* __restrict__ x, T* __restrict__ y, long long R, int C,
    float scale, int causal_seq, Lens<VARLEN> lens) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  constexpr int V = VecTraits<T>::kElems;
  const bool vec = softmax_vec(C, V);
  for (long long r = (long long)blockIdx.x * 4 + wid; r < R;
       r += (long long)gridDim.x * 4) {
    const T* row = x + r * C;
    T* yrow = y + r * C;
    int qpos = CAUSAL ? (int)(r % causal_seq) : C - 1;
    if constexpr (VARLEN) {
      qpos = len_limit(lens, r, C, qpos);
      if (qpos < 0) {   // wave-uniform
        if (vec) {
          float f[V] = {};
          for (int cv = lane; cv < C / V; cv += 64) vstore16(yrow + cv * V, f);
        } else {
          for (int c = lane; c < C; c += 64) yrow[c] = (T)0.f;
        }
        continue;
      }
    }
    float m = -INFINITY;
    if (vec) {
      for (int cv = lane; cv < C / V; cv += 64) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (cv * V + q <= qpos) m = fmaxf(m, f[q] * scale);
      }
    } else {
      for (int c = lane; c <= qpos; c += 64) m = fmaxf(m, (float)row[c] * scale);
    }
    m = wave_reduce_max(m);
    m = __shfl(m, 0, kWave);
    float acc = 0.f;
    if (vec) {
      for (int cv = lane; cv < C / V; cv += 64) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (cv * V + q <= qpos) acc += __expf(f[q] * scale - m);
      }
    } else {
      for (int c = lane; c <= qpos; c += 64) acc += __expf((float)row[c] * scale - m);
    }
    acc = wave_reduce_sum(acc);
    const float inv = 1.f / __shfl(acc, 0, kWave);
    if (vec) {
      for (int cv = lane; cv < C / V; cv += 64) {
        float f[V];
        vload16(row + cv * V, f);
#pragma unroll
        for (int q = 0; q < V; ++q)
          f[q] = cv * V + q <= qpos ? __expf(f[q] * scale - m) * inv : 0.f;
        vstore16(yrow + cv * V, f);
      }
    } else {
      for (int c = lane; c < C; c += 64)
        yrow[c] = (T)(c <= qpos ? __expf((float)row[c] * scale - m) * inv : 0.f);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void softmax_bwd_wave_kernel(
    const T* __restrict__ y, const T* __restrict__ dy, T* __restrict__ dx,
    long long R, int C, float scale) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  constexpr int V = VecTraits<T>::kElems;
  const bool vec = softmax_vec(C, V);
  for (long long r = (long long)blockIdx.x * 4 + wid; r < R;
       r += (long long)gridDim.x * 4) {
    const T* yrow = y + r * C;
    const T* dyrow = dy + r * C;
    T* dxrow = dx + r * C;
    float acc = 0.f;
    if (vec) {
      for (int cv = lane; cv < C / V; cv += 64) {
        float fy[V], fd[V];
        vload16(yrow + cv * V, fy);
        vload16(dyrow + cv * V, fd);
#pragma unroll
        for (int q = 0; q < V; ++q) acc = fmaf(fd[q], fy[q], acc);
      }
    } else {
      for (int c = lane; c < C; c += 64)
        acc = fmaf((float)dyrow[c], (float)yrow[c], acc);
    }
    acc = wave_reduce_sum(acc);
    const float dot = __shfl(acc, 0, kWave);
    if (vec) {
      for (int cv = lane; cv < C / V; cv += 64) {
        float fy[V], fd[V];
        vload16(yrow + cv * V, fy);
        vload16(dyrow + cv * V, fd);
#pragma unroll
        for (int q = 0; q < V; ++q) fd[q] = scale * fy[q] * (fd[q] - dot);
        vstore16(dxrow + cv * V, fd);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        float yv = (float)yrow[c];
        dxrow[c] = (T)(scale * yv * ((float)dyrow[c] - dot));
      }
    }
  }
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

// Kernel and grid come from softmax_route; kv_len == nullptr launches the
// dense instantiations.
void launch_softmax_fwd(bool is_bf16, const void* x, void* y, long long R,
                        int C, float scale, int causal_seq, const int* kv_len,
                        long long rows_per_len, int q_period, hipStream_t s) {
  const SoftmaxRoute rt = softmax_route(R, C, is_bf16);
  const RowLens lens{kv_len, rows_per_len, q_period};
  auto launch = [&](auto t, auto cz, auto vl) {
    using T = decltype(t);
    constexpr bool CZ = decltype(cz)::value, VL = decltype(vl)::value;
    Lens<VL> la;
    if constexpr (VL) la = lens;
    hipLaunchKernelGGL((rt.wave ? softmax_fwd_wave_kernel<T, CZ, VL>
                                : softmax_fwd_kernel<T, CZ, VL>),
                       dim3(rt.grid), dim3(kBlock), 0, s, (const T*)x, (T*)y,
                       R, C, scale, causal_seq, la);
  };
  dispatch2(causal_seq > 0, kv_len != nullptr, [&](auto cz, auto vl) {
    if (is_bf16) launch(bf16{}, cz, vl); else launch(float{}, cz, vl);
  });
}

void launch_softmax_bwd(bool is_bf16, const void* y, const void* dy, void* dx,
                        long long R, int C, float scale, hipStream_t s) {
  const SoftmaxRoute rt = softmax_route(R, C, is_bf16);
  auto launch = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(
        (rt.wave ? softmax_bwd_wave_kernel<T> : softmax_bwd_kernel<T>),
        dim3(rt.grid), dim3(kBlock), 0, s, (const T*)y, (const T*)dy, (T*)dx,
        R, C, scale);
  };
  if (is_bf16) launch(bf16{}); else launch(float{});
}

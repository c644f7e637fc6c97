// Loss kernels (gfx950): MSE and cross-entropy, forward + backward.
//
// Both are fused single-pass kernels: MSE is a reduce over flat_walk
// (common.h); CE (the classifier configs, ResNet/BERT) is one block per row
// with an online log-sum-exp (no materialized softmax in the forward).
#include "common.h"

// ---- MSE ------------------------------------------------------------------

// partial = sum((x-y)^2); out[0] += partial (atomic). Caller zeroes out and
// divides by n (mean) on device via the tiny finalize kernel below. A thread
// chains its fmas in flat_walk's order.
template <typename T>
__global__ void mse_fwd_kernel(const T* __restrict__ x, const T* __restrict__ y,
                               float* __restrict__ out, long long n) {
  __shared__ float scratch[kBlock / kWave];
  float acc = 0.f;
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float xf[W], yf[W];
    vload<W>(x + e, xf);
    vload<W>(y + e, yf);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float d = xf[k] - yf[k];
      acc = fmaf(d, d, acc);
    }
  });
  float total = block_reduce_sum(acc, scratch);
  if (threadIdx.x == 0) atomicAdd(out, total);
}

__global__ void scale_scalar_kernel(float* __restrict__ out, float scale) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] *= scale;
}

// dx = 2*(x-y)/n * dout   (dout is a device scalar)
template <typename T>
__global__ void mse_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y,
                               const float* __restrict__ dout,
                               T* __restrict__ dx, long long n) {
  const float c = 2.f * dout[0] / (float)n;
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float xf[W], yf[W];
    vload<W>(x + e, xf);
    vload<W>(y + e, yf);
#pragma unroll
    for (int k = 0; k < W; ++k) xf[k] = c * (xf[k] - yf[k]);
    vstore<W>(dx + e, xf);
  });
}

// ---- Cross-entropy ---------------------------------------------------------

// Ignored labels. The MASKED instantiations take a CeMask as their last
// argument: row b is live iff 0 <= target[b] < C and target[b] != ignore_index,
// every other row is ignored: its logits are never read, its lse and dx row are
// stored as +0.0, and it adds nothing to loss_sum or to the live-row count
// n_valid. A label outside [0, C) therefore never becomes an address. The
// dense instantiations take no such argument at all (an empty pack: even an
// empty struct would move the hidden arguments behind the 8-byte-aligned
// explicit ones), so they keep their code and their argument block.
struct CeMask {
  long long ignore_index;
  int* n_valid;  // [1]: live rows, counted by the forward, read by the backward
};
DEVINL const CeMask& ce_mask(const CeMask& m) { return m; }

DEVINL bool ce_live(long long t, int C, long long ignore_index) {
  return t >= 0 && t < (long long)C && t != ignore_index;
}

// One block per row. Two passes over the row (max, then sum-exp), both
// block-reduced; stores per-row lse and the row loss; loss_sum accumulated
// atomically by the caller-side finalize (mean).
template <typename T, bool MASKED, typename... Mask>
__global__ void ce_fwd_kernel(const T* __restrict__ logits,
                              const long long* __restrict__ target,
                              float* __restrict__ lse,      // [B] saved for bwd
                              float* __restrict__ loss_sum, // [1]
                              int B, int C, Mask... mask) {
  static_assert(sizeof...(Mask) == (MASKED ? 1 : 0), "MASKED takes one CeMask");
  __shared__ float scratch[kBlock / kWave];
  __shared__ float s_max, s_sum;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    if constexpr (MASKED) {
      // target[b] is block-uniform: the whole block skips the row and every
      // barrier below with it, so the barriers of the next trip stay matched
      if (!ce_live(target[b], C, ce_mask(mask...).ignore_index)) {
        if (threadIdx.x == 0) lse[b] = 0.f;
        continue;
      }
    }
    const T* row = logits + (long long)b * C;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      m = fmaxf(m, (float)row[c]);
    // block max via sum-scratch trick (reuse block_reduce with max)
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
    float m_all = s_max;
    float acc = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      acc += __expf((float)row[c] - m_all);
    float sum = block_reduce_sum(acc, scratch);
    if (threadIdx.x == 0) {
      s_sum = sum;
      float row_lse = m_all + __logf(sum);
      lse[b] = row_lse;
      float t_logit = (float)row[target[b]];
      atomicAdd(loss_sum, row_lse - t_logit);
      if constexpr (MASKED) atomicAdd(ce_mask(mask...).n_valid, 1);
    }
    __syncthreads();
  }
}

// loss = loss_sum / n_valid on the device (no host read: a captured graph can
// carry it); a minibatch without a live row has loss 0, not 0 / 0.
__global__ void ce_masked_finalize_kernel(float* __restrict__ loss,
                                          const int* __restrict__ n_valid) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int n = n_valid[0];
    loss[0] = n > 0 ? loss[0] / (float)n : 0.0f;
  }
}

// dx[b,c] = (softmax - onehot) * dout / B; MASKED: / n_valid over the live
// rows, +0.0 over the ignored ones
template <typename T, bool MASKED, typename... Mask>
__global__ void ce_bwd_kernel(const T* __restrict__ logits,
                              const long long* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ dout,
                              T* __restrict__ dx, int B, int C, Mask... mask) {
  static_assert(sizeof...(Mask) == (MASKED ? 1 : 0), "MASKED takes one CeMask");
  float scale;
  if constexpr (MASKED) {
    const int n = ce_mask(mask...).n_valid[0];
    scale = n > 0 ? dout[0] / (float)n : 0.f;
  } else {
    scale = dout[0] / (float)B;
  }
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const T* row = logits + (long long)b * C;
    T* drow = dx + (long long)b * C;
    const float row_lse = lse[b];
    const long long t = target[b];
    if constexpr (MASKED) {
      if (!ce_live(t, C, ce_mask(mask...).ignore_index)) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) drow[c] = (T)0.f;
        continue;
      }
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float p = __expf((float)row[c] - row_lse);
      drow[c] = (T)(scale * (p - (c == t ? 1.f : 0.f)));
    }
  }
}

#define CE_INSTANTIATE(T)                                                      \
  template __global__ void ce_fwd_kernel<T, false>(                            \
      const T*, const long long*, float*, float*, int, int);                   \
  template __global__ void ce_fwd_kernel<T, true, CeMask>(                     \
      const T*, const long long*, float*, float*, int, int, CeMask);           \
  template __global__ void ce_bwd_kernel<T, false>(                            \
      const T*, const long long*, const float*, const float*, T*, int, int);   \
  template __global__ void ce_bwd_kernel<T, true, CeMask>(                     \
      const T*, const long long*, const float*, const float*, T*, int, int,    \
      CeMask);
CE_INSTANTIATE(float)
CE_INSTANTIATE(bf16)
#undef CE_INSTANTIATE

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

void launch_mse_fwd(bool is_bf16, const void* x, const void* y, float* out,
                    long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(mse_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)x, (const T*)y, out, n);
  });
}

void launch_scale_scalar(float* out, float scale, hipStream_t s) {
  hipLaunchKernelGGL(scale_scalar_kernel, dim3(1), dim3(64), 0, s, out, scale);
}

void launch_mse_bwd(bool is_bf16, const void* x, const void* y,
                    const float* dout, void* dx, long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(mse_bwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)x, (const T*)y, dout, (T*)dx, n);
  });
}

void launch_ce_fwd(bool is_bf16, const void* logits, const long long* target,
                   float* lse, float* loss_sum, int B, int C, hipStream_t s) {
  const int grid = B < kMaxGrid ? B : kMaxGrid;
  if (is_bf16)
    hipLaunchKernelGGL((ce_fwd_kernel<bf16, false>), dim3(grid), dim3(kBlock),
                       0, s, (const bf16*)logits, target, lse, loss_sum, B, C);
  else
    hipLaunchKernelGGL((ce_fwd_kernel<float, false>), dim3(grid), dim3(kBlock),
                       0, s, (const float*)logits, target, lse, loss_sum, B, C);
}

void launch_ce_bwd(bool is_bf16, const void* logits, const long long* target,
                   const float* lse, const float* dout, void* dx, int B, int C,
                   hipStream_t s) {
  const int grid = B < kMaxGrid ? B : kMaxGrid;
  if (is_bf16)
    hipLaunchKernelGGL((ce_bwd_kernel<bf16, false>), dim3(grid), dim3(kBlock),
                       0, s, (const bf16*)logits, target, lse, dout, (bf16*)dx,
                       B, C);
  else
    hipLaunchKernelGGL((ce_bwd_kernel<float, false>), dim3(grid), dim3(kBlock),
                       0, s, (const float*)logits, target, lse, dout,
                       (float*)dx, B, C);
}

// loss holds the sum over the live rows after the row kernel; the one-thread
// finalize turns it into their mean on the same stream.
void launch_ce_masked_fwd(bool is_bf16, const void* logits,
                          const long long* target, float* lse, float* loss,
                          int* n_valid, long long ignore_index, int B, int C,
                          hipStream_t s) {
  const int grid = B < kMaxGrid ? B : kMaxGrid;
  const CeMask mask{ignore_index, n_valid};
  if (is_bf16)
    hipLaunchKernelGGL((ce_fwd_kernel<bf16, true, CeMask>), dim3(grid), dim3(kBlock), 0,
                       s, (const bf16*)logits, target, lse, loss, B, C, mask);
  else
    hipLaunchKernelGGL((ce_fwd_kernel<float, true, CeMask>), dim3(grid), dim3(kBlock),
                       0, s, (const float*)logits, target, lse, loss, B, C,
                       mask);
  hipLaunchKernelGGL(ce_masked_finalize_kernel, dim3(1), dim3(64), 0, s, loss,
                     (const int*)n_valid);
}

void launch_ce_masked_bwd(bool is_bf16, const void* logits,
                          const long long* target, const float* lse,
                          const int* n_valid, const float* dout, void* dx,
                          long long ignore_index, int B, int C, hipStream_t s) {
  const int grid = B < kMaxGrid ? B : kMaxGrid;
  const CeMask mask{ignore_index, const_cast<int*>(n_valid)};
  if (is_bf16)
    hipLaunchKernelGGL((ce_bwd_kernel<bf16, true, CeMask>), dim3(grid), dim3(kBlock), 0,
                       s, (const bf16*)logits, target, lse, dout, (bf16*)dx, B,
                       C, mask);
  else
    hipLaunchKernelGGL((ce_bwd_kernel<float, true, CeMask>), dim3(grid), dim3(kBlock),
                       0, s, (const float*)logits, target, lse, dout,
                       (float*)dx, B, C, mask);
}

// Elementwise kernels (gfx950): ReLU, residual add+ReLU, GELU — the glue
// ops of the model zoo. A kernel is one body over flat_walk (common.h); the
// two GELU kernels keep their own loops (note at gelu_fwd_kernel).
#include "common.h"

template <typename T>
__global__ void relu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float f[W];
    vload<W>(x + e, f);
#pragma unroll
    for (int k = 0; k < W; ++k) f[k] = fmaxf(f[k], 0.f);
    vstore<W>(y + e, f);
  });
}

// dx = dy * (y > 0)
template <typename T>
__global__ void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                T* __restrict__ dx, long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float df[W], yf[W];
    if constexpr (W == 1) {
      // the tail reads dy only where y > 0, as it always has
      vload<W>(y + e, yf);
      df[0] = yf[0] > 0.f ? (float)dy[e] : 0.f;
    } else {
      vload<W>(dy + e, df);
      vload<W>(y + e, yf);
#pragma unroll
      for (int k = 0; k < W; ++k) df[k] = yf[k] > 0.f ? df[k] : 0.f;
    }
    vstore<W>(dx + e, df);
  });
}

// y = relu(a + b) — the ResNet residual join, fused
template <typename T>
__global__ void add_relu_fwd_kernel(const T* __restrict__ a,
                                    const T* __restrict__ b, T* __restrict__ y,
                                    long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float af[W], bf[W];
    vload<W>(a + e, af);
    vload<W>(b + e, bf);
#pragma unroll
    for (int k = 0; k < W; ++k) af[k] = fmaxf(af[k] + bf[k], 0.f);
    vstore<W>(y + e, af);
  });
}

// z = a + alpha * b — the LoRA combine (base + scaling * delta), fused:
// one kernel instead of a scale pass plus an add pass (3 tensor passes
// instead of 5 at ~6 TB/s HBM-bound)
template <typename T>
__global__ void add_scaled_fwd_kernel(const T* __restrict__ a,
                                      const T* __restrict__ b,
                                      T* __restrict__ z, float alpha,
                                      long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float af[W], bf[W];
    vload<W>(a + e, af);
    vload<W>(b + e, bf);
#pragma unroll
    for (int k = 0; k < W; ++k) af[k] = fmaf(alpha, bf[k], af[k]);
    vstore<W>(z + e, af);
  });
}

// z = alpha * x (the add_scaled backward for the delta operand)
template <typename T>
__global__ void scale_fwd_kernel(const T* __restrict__ x, T* __restrict__ z,
                                 float alpha, long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float f[W];
    vload<W>(x + e, f);
#pragma unroll
    for (int k = 0; k < W; ++k) f[k] *= alpha;
    vstore<W>(z + e, f);
  });
}

// tanh-approx GELU (BERT): y = 0.5x(1+tanh(0.79788456(x+0.044715x^3)))
DEVINL float gelu_of(float v) {
  float inner = 0.7978845608f * fmaf(0.044715f * v * v, v, v);
  return 0.5f * v * (1.f + tanhf(inner));
}

// Hand-written: over flat_walk the compiler packs the arithmetic after tanhf
// (v_pk_*), another instruction mix and up to 8 more VGPRs (gelu_bwd<bf16>).
template <typename T>
__global__ void gelu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                long long n) {
  constexpr int V = VecTraits<T>::kElems;
  const long long nvec = n / V;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    float f[V];
    vload16(x + i * V, f);
#pragma unroll
    for (int q = 0; q < V; ++q) f[q] = gelu_of(f[q]);
    vstore16(y + i * V, f);
  }
  for (long long i = nvec * V + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x)
    y[i] = (T)gelu_of((float)x[i]);
}

DEVINL float gelu_grad(float v) {
  float inner = 0.7978845608f * fmaf(0.044715f * v * v, v, v);
  float t = tanhf(inner);
  float dinner = 0.7978845608f * fmaf(3.f * 0.044715f * v, v, 1.f);
  return 0.5f * (1.f + t) + 0.5f * v * (1.f - t * t) * dinner;
}

// Hand-written, see gelu_fwd_kernel.
template <typename T>
__global__ void gelu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                T* __restrict__ dx, long long n) {
  constexpr int V = VecTraits<T>::kElems;
  const long long nvec = n / V;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    float fx[V], fd[V];
    vload16(x + i * V, fx);
    vload16(dy + i * V, fd);
#pragma unroll
    for (int q = 0; q < V; ++q) fd[q] *= gelu_grad(fx[q]);
    vstore16(dx + i * V, fd);
  }
  for (long long i = nvec * V + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x)
    dx[i] = (T)((float)dy[i] * gelu_grad((float)x[i]));
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

void launch_relu_fwd(bool is_bf16, const void* x, void* y, long long n,
                     hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(relu_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)x, (T*)y, n);
  });
}

void launch_relu_bwd(bool is_bf16, const void* dy, const void* y, void* dx,
                     long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)dy, (const T*)y, (T*)dx, n);
  });
}

void launch_add_relu_fwd(bool is_bf16, const void* a, const void* b, void* y,
                         long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(add_relu_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)a, (const T*)b, (T*)y, n);
  });
}

void launch_add_scaled_fwd(bool is_bf16, const void* a, const void* b, void* z,
                           float alpha, long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(add_scaled_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0,
                       s, (const T*)a, (const T*)b, (T*)z, alpha, n);
  });
}

void launch_scale_fwd(bool is_bf16, const void* x, void* z, float alpha,
                      long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 8 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(scale_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)x, (T*)z, alpha, n);
  });
}

void launch_gelu_fwd(bool is_bf16, const void* x, void* y, long long n,
                     hipStream_t s) {
  const int grid = elementwise_grid(n / 4 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(gelu_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)x, (T*)y, n);
  });
}

void launch_gelu_bwd(bool is_bf16, const void* dy, const void* x, void* dx,
                     long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 4 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(gelu_bwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)dy, (const T*)x, (T*)dx, n);
  });
}

// Llama-family kernels (gfx950): RoPE, SwiGLU — fwd + bwd. (RMSNorm shares
// LayerNorm's kernels in norm.hip.)
//
// BASELINE.json config 4 (Llama-3-8B LoRA federated fine-tune). Both are
// memory-bound streaming ops in fp32 math: SwiGLU is two bodies over flat_walk
// (common.h), RoPE a grid-stride loop over pairs. RoPE uses host-precomputed
// cos/sin tables (guide Appendix B: on-device trig turns a memory-bound op
// VALU-bound).
#include "common.h"

// ---- RoPE (neox half-rotation) ---------------------------------------------
// x: [..., S, H, D] contiguous; pair (d, d+D/2) rotated by angle tables
// cos/sin [S, D/2] fp32. FWD=false applies the inverse rotation (backward).

template <typename T, bool INV>
__global__ void rope_kernel(const T* __restrict__ x, T* __restrict__ y,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t, long long total,
                            int S, int H, int D) {
  const int half = D / 2;
  const long long pairs_per_s = (long long)H * half;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    // i indexes (b, s, h, d<half)
    const int d = (int)(i % half);
    const long long t = i / half;
    const int h = (int)(t % H);
    const long long t2 = t / H;
    const int s = (int)(t2 % S);
    const long long b = t2 / S;
    const long long base = ((b * S + s) * H + h) * (long long)D + d;
    const float c = cos_t[s * half + d];
    const float sn = sin_t[s * half + d];
    const float x1 = (float)x[base];
    const float x2 = (float)x[base + half];
    if (INV) {
      y[base] = (T)fmaf(x1, c, x2 * sn);
      y[base + half] = (T)fmaf(x2, c, -x1 * sn);
    } else {
      y[base] = (T)fmaf(x1, c, -x2 * sn);
      y[base + half] = (T)fmaf(x1, sn, x2 * c);
    }
  }
}

// ---- SwiGLU ----------------------------------------------------------------
// fwd: y = silu(a) * b;  bwd: da = dy*b*silu'(a), db = dy*silu(a)

template <typename T>
__global__ void silu_mul_fwd_kernel(const T* __restrict__ a,
                                    const T* __restrict__ b, T* __restrict__ y,
                                    long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float fa[W], fb[W];
    vload<W>(a + e, fa);
    vload<W>(b + e, fb);
#pragma unroll
    for (int q = 0; q < W; ++q) {
      float sig = 1.f / (1.f + __expf(-fa[q]));
      fa[q] = fa[q] * sig * fb[q];
    }
    vstore<W>(y + e, fa);
  });
}

template <typename T>
__global__ void silu_mul_bwd_kernel(const T* __restrict__ dy,
                                    const T* __restrict__ a,
                                    const T* __restrict__ b, T* __restrict__ da,
                                    T* __restrict__ db, long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float fa[W], fb[W], fd[W], fda[W], fdb[W];
    vload<W>(a + e, fa);
    vload<W>(b + e, fb);
    vload<W>(dy + e, fd);
#pragma unroll
    for (int q = 0; q < W; ++q) {
      float sig = 1.f / (1.f + __expf(-fa[q]));
      float silu = fa[q] * sig;
      float dsilu = sig * fmaf(fa[q], 1.f - sig, 1.f);
      fda[q] = fd[q] * fb[q] * dsilu;
      fdb[q] = fd[q] * silu;
    }
    vstore<W>(da + e, fda);
    vstore<W>(db + e, fdb);
  });
}

#define INST_LLAMA(T)                                                          \
  template __global__ void rope_kernel<T, false>(const T*, T*, const float*,   \
                                                 const float*, long long, int, \
                                                 int, int);                    \
  template __global__ void rope_kernel<T, true>(const T*, T*, const float*,    \
                                                const float*, long long, int,  \
                                                int, int);

INST_LLAMA(float)
INST_LLAMA(bf16)

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

void launch_rope(bool is_bf16, bool inverse, const void* x, void* y,
                 const float* cos_t, const float* sin_t, long long total_pairs,
                 int S, int H, int D, hipStream_t s) {
  const int grid = elementwise_grid(total_pairs);
  #define ROPE_CALL(T, I)                                                     \
    hipLaunchKernelGGL((rope_kernel<T, I>), dim3(grid), dim3(kBlock), 0, s,   \
                       (const T*)x, (T*)y, cos_t, sin_t, total_pairs, S, H, D)
  if (is_bf16) { if (inverse) ROPE_CALL(bf16, true); else ROPE_CALL(bf16, false); }
  else { if (inverse) ROPE_CALL(float, true); else ROPE_CALL(float, false); }
  #undef ROPE_CALL
}

void launch_silu_mul_fwd(bool is_bf16, const void* a, const void* b, void* y,
                         long long n, hipStream_t s) {
  const int grid = elementwise_grid(n / 4 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(silu_mul_fwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)a, (const T*)b, (T*)y, n);
  });
}

void launch_silu_mul_bwd(bool is_bf16, const void* dy, const void* a,
                         const void* b, void* da, void* db, long long n,
                         hipStream_t s) {
  const int grid = elementwise_grid(n / 4 + 1);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(silu_mul_bwd_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)dy, (const T*)a, (const T*)b, (T*)da, (T*)db,
                       n);
  });
}

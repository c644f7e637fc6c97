// Fused optimizer kernels (gfx950).
//
// The whole step is one HBM-rate streaming kernel over a flat buffer
// (runtime/arena.py): p/g in fp32 or bf16, momentum/Adam moments always fp32.
// grad_sumsq and the zero fill are bodies over flat_walk (common.h) on
// optim_grid blocks; the two step kernels walk the same way by hand (note at
// sgd_kernel). No host sync.
#include "common.h"

// Clipping, the non-finite skip and decoupled decay. The EXT instantiations
// take an OptExt as their last argument; the dense ones take an empty pack
// (not an empty struct, which would move the hidden arguments), so they keep
// their argument block and their code.
//   clip_state (may be null) is the vector clip_finalize_kernel writes:
//     [0] norm  [1] coef  [2] 1.0 finite / 0.0 not  [3] skipped steps so far
//   [2] == 0: the step is skipped, a uniform early exit in front of all
//     arithmetic (coef is 0 then, and 0 * inf must never be formed): p, m, v
//     are not written, g is still zeroed under zero_after.
//   otherwise g' = coef * g, one fp32 multiply of its own, and then
//     decoupled == 0: the dense arithmetic on g'
//     decoupled == 1: p = fma(-lr * wd, p, p), then the update from g' with
//                     no L2 term (torch.optim.AdamW; torch's form for SGD)
struct OptExt {
  const float* clip_state;
  int decoupled;
};
DEVINL const OptExt& opt_ext(const OptExt& e) { return e; }

// The gradient an EXT step consumes; p is decayed in place when decoupled.
DEVINL float ext_grad(float g, float& p, float coef, bool decoupled,
                      float decay, float weight_decay) {
  const float gc = coef * g;
  if (decoupled) {
    p = fmaf(decay, p, p);
    return gc;
  }
  return fmaf(weight_decay, p, gc);
}

// A skipped step's only work: the fused zero_grad.
template <typename T>
DEVINL void zero_grads(T* __restrict__ g, long long n) {
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    vzero<decltype(w)::value>(g + e);
  });
}

// sgd_kernel and adam_kernel keep their own loops: over flat_walk sgd's tail
// no longer shares its update of p between the momentum branches (one fma
// more), and adam<float, EXT> takes 5 more VGPRs with another packed-math mix.
// zero_after: write zeros back to g after consuming it — fuses the next
// iteration's zero_grad fill into this pass (one launch fewer per step).
template <typename T, bool EXT, typename... Ext>
__global__ void sgd_kernel(T* __restrict__ p, T* __restrict__ g,
                           float* __restrict__ m, long long n, float lr,
                           float momentum, float weight_decay,
                           int zero_after, Ext... ext) {
  static_assert(sizeof...(Ext) == (EXT ? 1 : 0), "EXT takes one OptExt");
  using VT = VecTraits<T>;
  constexpr int V = VT::kElems;
  const long long nvec = n / V;
  const bool has_m = (m != nullptr);
  [[maybe_unused]] float coef = 1.f, decay = 0.f;
  [[maybe_unused]] bool decoupled = false;
  if constexpr (EXT) {
    const OptExt& e = opt_ext(ext...);
    if (e.clip_state != nullptr) {
      if (e.clip_state[2] == 0.f) {
        if (zero_after) zero_grads(g, n);
        return;
      }
      coef = e.clip_state[1];
    }
    decoupled = e.decoupled != 0;
    decay = -lr * weight_decay;
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    typename VT::VecT pv = reinterpret_cast<const typename VT::VecT*>(p)[i];
    typename VT::VecT gv = reinterpret_cast<const typename VT::VecT*>(g)[i];
    float pf[V], gf[V];
    VT::to_float(pv, pf);
    VT::to_float(gv, gf);
    if (has_m) {
      f32x4 mv[V / 4];
#pragma unroll
      for (int q = 0; q < V / 4; ++q)
        mv[q] = reinterpret_cast<const f32x4*>(m)[i * (V / 4) + q];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float grad;
        if constexpr (EXT)
          grad = ext_grad(gf[k], pf[k], coef, decoupled, decay, weight_decay);
        else
          grad = fmaf(weight_decay, pf[k], gf[k]);
        float mom = fmaf(momentum, mv[k / 4][k % 4], grad);
        mv[k / 4][k % 4] = mom;
        pf[k] = fmaf(-lr, mom, pf[k]);
      }
#pragma unroll
      for (int q = 0; q < V / 4; ++q)
        reinterpret_cast<f32x4*>(m)[i * (V / 4) + q] = mv[q];
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float grad;
        if constexpr (EXT)
          grad = ext_grad(gf[k], pf[k], coef, decoupled, decay, weight_decay);
        else
          grad = fmaf(weight_decay, pf[k], gf[k]);
        pf[k] = fmaf(-lr, grad, pf[k]);
      }
    }
    VT::from_float(pf, pv);
    reinterpret_cast<typename VT::VecT*>(p)[i] = pv;
    if (zero_after)
      reinterpret_cast<typename VT::VecT*>(g)[i] = typename VT::VecT{};
  }
  // scalar tail
  long long tail_start = nvec * V;
  for (long long i = tail_start + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float pf = (float)p[i], gf = (float)g[i];
    float grad;
    if constexpr (EXT)
      grad = ext_grad(gf, pf, coef, decoupled, decay, weight_decay);
    else
      grad = fmaf(weight_decay, pf, gf);
    if (has_m) {
      float mom = fmaf(momentum, m[i], grad);
      m[i] = mom;
      grad = mom;
    }
    p[i] = (T)fmaf(-lr, grad, pf);
    if (zero_after) g[i] = (T)0.f;
  }
}

template <typename T, bool EXT, typename... Ext>
__global__ void adam_kernel(T* __restrict__ p, T* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            long long n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float inv_bc1,
                            float inv_sqrt_bc2, int zero_after, Ext... ext) {
  static_assert(sizeof...(Ext) == (EXT ? 1 : 0), "EXT takes one OptExt");
  using VT = VecTraits<T>;
  constexpr int V = VT::kElems;
  const long long nvec = n / V;
  [[maybe_unused]] float coef = 1.f, decay = 0.f;
  [[maybe_unused]] bool decoupled = false;
  if constexpr (EXT) {
    const OptExt& e = opt_ext(ext...);
    if (e.clip_state != nullptr) {
      if (e.clip_state[2] == 0.f) {
        if (zero_after) zero_grads(g, n);
        return;
      }
      coef = e.clip_state[1];
    }
    decoupled = e.decoupled != 0;
    decay = -lr * weight_decay;
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    typename VT::VecT pv = reinterpret_cast<const typename VT::VecT*>(p)[i];
    typename VT::VecT gv = reinterpret_cast<const typename VT::VecT*>(g)[i];
    float pf[V], gf[V];
    VT::to_float(pv, pf);
    VT::to_float(gv, gf);
    f32x4 mv[V / 4], vv[V / 4];
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      mv[q] = reinterpret_cast<const f32x4*>(m)[i * (V / 4) + q];
      vv[q] = reinterpret_cast<const f32x4*>(v)[i * (V / 4) + q];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float grad;
      if constexpr (EXT)
        grad = ext_grad(gf[k], pf[k], coef, decoupled, decay, weight_decay);
      else
        grad = fmaf(weight_decay, pf[k], gf[k]);
      float m_new = fmaf(beta1, mv[k / 4][k % 4], (1.f - beta1) * grad);
      float v_new = fmaf(beta2, vv[k / 4][k % 4], (1.f - beta2) * grad * grad);
      mv[k / 4][k % 4] = m_new;
      vv[k / 4][k % 4] = v_new;
      // p -= lr * (m/bc1) / (sqrt(v/bc2) + eps)
      float denom = fmaf(sqrtf(v_new), inv_sqrt_bc2, eps);
      pf[k] = fmaf(-lr * inv_bc1, m_new / denom, pf[k]);
    }
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      reinterpret_cast<f32x4*>(m)[i * (V / 4) + q] = mv[q];
      reinterpret_cast<f32x4*>(v)[i * (V / 4) + q] = vv[q];
    }
    VT::from_float(pf, pv);
    reinterpret_cast<typename VT::VecT*>(p)[i] = pv;
    if (zero_after)
      reinterpret_cast<typename VT::VecT*>(g)[i] = typename VT::VecT{};
  }
  long long tail_start = nvec * V;
  for (long long i = tail_start + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float pf = (float)p[i], gf = (float)g[i];
    float grad;
    if constexpr (EXT)
      grad = ext_grad(gf, pf, coef, decoupled, decay, weight_decay);
    else
      grad = fmaf(weight_decay, pf, gf);
    float m_new = fmaf(beta1, m[i], (1.f - beta1) * grad);
    float v_new = fmaf(beta2, v[i], (1.f - beta2) * grad * grad);
    m[i] = m_new;
    v[i] = v_new;
    float denom = fmaf(sqrtf(v_new), inv_sqrt_bc2, eps);
    p[i] = (T)fmaf(-lr * inv_bc1, m_new / denom, pf);
    if (zero_after) g[i] = (T)0.f;
  }
}

// ---- global gradient norm ---------------------------------------------------
// Stage 1: every thread chains fma(x, x, acc) over its elements in fp32, in
// flat_walk's order, the block reduces (6 shuffle levels, then the 4 wave sums
// in order) and stores ONE partial at partials[blockIdx.x]. No atomics: the
// norm has the same bits in every run.
template <typename T>
__global__ void grad_sumsq_kernel(const T* __restrict__ g, long long n,
                                  float* __restrict__ partials) {
  __shared__ float scratch[kBlock / kWave];
  float acc = 0.f;
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float gf[W];
    vload<W>(g + e, gf);
#pragma unroll
    for (int k = 0; k < W; ++k) acc = fmaf(gf[k], gf[k], acc);
  });
  const float total = block_reduce_sum(acc, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Stage 2, one block: thread t adds partials t, t + 256, ... in fp64, then a
// fixed binary tree over the 256 sums in LDS. Thread 0 turns the total into
// clip_state (see OptExt); [3] counts the skipped steps and is only ever
// incremented here.
__global__ void clip_finalize_kernel(const float* __restrict__ partials,
                                     int count, double max_norm,
                                     float* __restrict__ clip_state) {
  __shared__ double red[kBlock];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += kBlock) acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sumsq = red[0];
    const bool finite = isfinite(sumsq);
    const double norm = sqrt(sumsq);
    // torch's clip_grad_norm_ rule, in fp64, rounded once
    const double c = fmin(1.0, max_norm / (norm + 1e-6));
    const float skipped = clip_state[3];
    clip_state[0] = (float)norm;
    clip_state[1] = finite ? (float)c : 0.f;
    clip_state[2] = finite ? 1.f : 0.f;
    clip_state[3] = finite ? skipped : skipped + 1.f;
  }
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

int optim_grid(long long n) { return elementwise_grid(n / 8 + 1); }

void launch_sgd(bool is_bf16, void* p, void* g, float* m, long long n,
                float lr, float momentum, float wd, int zero_after,
                hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((sgd_kernel<T, false>), dim3(grid), dim3(kBlock), 0, s,
                       (T*)p, (T*)g, m, n, lr, momentum, wd, zero_after);
  });
}

void launch_adam(bool is_bf16, void* p, void* g, float* m, float* v,
                 long long n, float lr, float b1, float b2, float eps, float wd,
                 float inv_bc1, float inv_sqrt_bc2, int zero_after,
                 hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((adam_kernel<T, false>), dim3(grid), dim3(kBlock), 0, s,
                       (T*)p, (T*)g, m, v, n, lr, b1, b2, eps, wd, inv_bc1,
                       inv_sqrt_bc2, zero_after);
  });
}

void launch_sgd_ext(bool is_bf16, void* p, void* g, float* m, long long n,
                    float lr, float momentum, float wd, int zero_after,
                    const float* clip_state, int decoupled, hipStream_t s) {
  const int grid = optim_grid(n);
  const OptExt e{clip_state, decoupled};
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((sgd_kernel<T, true, OptExt>), dim3(grid), dim3(kBlock),
                       0, s, (T*)p, (T*)g, m, n, lr, momentum, wd, zero_after,
                       e);
  });
}

void launch_adam_ext(bool is_bf16, void* p, void* g, float* m, float* v,
                     long long n, float lr, float b1, float b2, float eps,
                     float wd, float inv_bc1, float inv_sqrt_bc2,
                     int zero_after, const float* clip_state, int decoupled,
                     hipStream_t s) {
  const int grid = optim_grid(n);
  const OptExt e{clip_state, decoupled};
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((adam_kernel<T, true, OptExt>), dim3(grid), dim3(kBlock),
                       0, s, (T*)p, (T*)g, m, v, n, lr, b1, b2, eps, wd,
                       inv_bc1, inv_sqrt_bc2, zero_after, e);
  });
}

int launch_grad_sumsq(bool is_bf16, const void* g, long long n,
                      float* partials, hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(grad_sumsq_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)g, n, partials);
  });
  return grid;
}

void launch_clip_finalize(const float* partials, int count, double max_norm,
                          float* clip_state, hipStream_t s) {
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kBlock), 0, s,
                     partials, count, max_norm, clip_state);
}

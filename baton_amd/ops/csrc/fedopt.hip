// Federated server step (gfx950): clipped client updates and the server
// optimizers of Reddi et al., "Adaptive Federated Optimization".
//
// Per round, with x the fp32 global model and theta a client's model in its
// own dtype, every client forms d = float(theta) - x, measures ||d||
// (delta_sumsq_kernel, then optim.hip's clip_finalize_kernel), and sends
// alpha * coef * d into the fp32 reduce buffer (delta_scale_cast_kernel); a
// client whose norm is not finite sends +0.0 and weight 0. The root turns the
// reduced weight W into round_state (fedopt_finalize_kernel) and applies
// Delta = D / W to x, m and v (server_step_kernel). All state is fp32, the
// kernels run flat_walk's geometry (common.h) on optim_grid blocks, the client
// side as bodies over it and the server step by hand (note at
// dp_noise_kernel), and nothing is read back by the host.
//
// DP-FedAvg (server_step_kernel<MODE, true>, dp_noise_kernel): Delta =
// fl(D + xi) with xi = fl(sigma * zeta) and zeta the Philox4x32-10 unit normal
// of (seed, round, stream, element), made in registers inside the same pass.
// The definition (counter layout, uniforms, Box-Muller, the fixed denominator
// and what the guarantee leaves out) is the docstring of fed/server_opt.py.
#include "common.h"

// Every operation below is rounded on its own: no a * b + c written with
// operators may become an fma (the fmas are spelled fmaf).
#pragma clang fp contract(off)

// ---- client side -----------------------------------------------------------

// grad_sumsq_kernel on float(theta) - x: every thread chains fma(d, d, acc)
// over its elements in flat_walk's order; one partial per block at
// partials[blockIdx.x], no atomics.
template <typename T>
__global__ void delta_sumsq_kernel(const T* __restrict__ theta,
                                   const float* __restrict__ x, long long n,
                                   float* __restrict__ partials) {
  __shared__ float scratch[kBlock / kWave];
  float acc = 0.f;
  flat_walk<VecTraits<T>::kElems>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float tf[W], xf[W];
    vload<W>(theta + e, tf);
    vload<W>(x + e, xf);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float d = tf[k] - xf[k];
      acc = fmaf(d, d, acc);
    }
  });
  const float total = block_reduce_sum(acc, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// dst = (alpha * coef) * (float(theta) - x), clip_state as clip_finalize
// wrote it. A non-finite client ([2] == 0) stores +0.0 and never reads theta:
// a uniform branch in front of the walk, so 0 * inf is never formed. w_out
// (may be null) receives the weight this client contributes to W.
template <typename T>
__global__ void delta_scale_cast_kernel(float* __restrict__ dst,
                                        const T* __restrict__ theta,
                                        const float* __restrict__ x,
                                        long long n, float alpha,
                                        const float* __restrict__ clip_state,
                                        float* __restrict__ w_out) {
  constexpr int V = VecTraits<T>::kElems;
  const bool finite = clip_state[2] != 0.f;
  if (w_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
    w_out[0] = finite ? alpha : 0.f;
  if (!finite) {
    flat_walk<V>(n, [&](long long e, auto w) {
      vzero<decltype(w)::value>(dst + e);
    });
    return;
  }
  const float s = alpha * clip_state[1];
  flat_walk<V>(n, [&](long long e, auto w) {
    constexpr int W = decltype(w)::value;
    float tf[W], xf[W];
    vload<W>(theta + e, tf);
    vload<W>(x + e, xf);
#pragma unroll
    for (int k = 0; k < W; ++k) tf[k] = s * (tf[k] - xf[k]);
    vstore<W>(dst + e, tf);
  });
}

// ---- server side -----------------------------------------------------------

// One thread: the reduced participation W -> round_state
//   [0] W  [1] inv_W = 1 / W in fp64, rounded once (0 on a skipped round)
//   [2] 1.0 applied / 0.0 skipped  [3] skipped rounds so far
// [3] is only ever incremented here.
__global__ void fedopt_finalize_kernel(const float* __restrict__ w_sum,
                                       float* __restrict__ round_state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float W = w_sum[0];
  const bool applied = isfinite(W) && W > 0.f;
  const float skipped = round_state[3];
  round_state[0] = W;
  round_state[1] = applied ? (float)(1.0 / (double)W) : 0.f;
  round_state[2] = applied ? 1.f : 0.f;
  round_state[3] = applied ? skipped : skipped + 1.f;
}

enum ServerMode : int {
  kServerMean = 0,     // x += Delta (float buffers; no momentum)
  kServerAvgM = 1,
  kServerAdagrad = 2,
  kServerAdam = 3,
  kServerYogi = 4,
};

// ---- DP noise: Philox4x32-10 and Box-Muller ----------------------------------

// What a noised launch adds to the server step: the key (lo32, hi32 of the
// seed), the round and stream words of the counter, the flat offset of
// element 0 within the stream (a multiple of 4) and the noise scale.
struct DpNoise {
  unsigned key0, key1, round, stream;
  long long elem_offset;
  float sigma;
};

// Philox4x32-10 with the Random123 constants: ten rounds, the key bumped by
// the Weyl increments between rounds.
DEVINL void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                          unsigned k0, unsigned k1, unsigned (&r)[4]) {
  constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr unsigned kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const unsigned hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kW0;
    k1 += kW1;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// Two unit normals from two words: u1 in (0, 1], u2 in [0, 1), both exact.
DEVINL void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(b >> 8) * 0x1p-24f;
  const float R = sqrtf(-2.f * logf(u1));
  const float t = 2.f * u2;
  z0 = R * cospif(t);
  z1 = R * sinpif(t);
}

// The four unit normals of block j (elements 4 j .. 4 j + 3 of the stream).
DEVINL void unit_normals4(const DpNoise& nz, long long j, float (&z)[4]) {
  unsigned r[4];
  philox4x32_10((unsigned)((unsigned long long)j & 0xFFFFFFFFull),
                (unsigned)((unsigned long long)j >> 32), nz.round, nz.stream,
                nz.key0, nz.key1, r);
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

// xi = fl(sigma * zeta) alone, on server_step_kernel's index walk: one Philox
// call per f32x4, the tail from block (elem_offset + n) >> 2.
// This kernel and server_step_kernel keep their own loops: here the tail's
// block is loop-invariant and its Philox call leaves the loop; over flat_walk
// it is recomputed per element (dp_noise 36 -> 52 VGPRs, twice the sqrt / log).
__global__ void dp_noise_kernel(float* __restrict__ out, long long n,
                                DpNoise nz) {
  const long long nvec = n / 4;
  const long long j0 = nz.elem_offset >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    float z[4];
    unit_normals4(nz, j0 + i, z);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = nz.sigma * z[k];
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
  for (long long i = nvec * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float z[4];
    unit_normals4(nz, j0 + nvec, z);
    const int lane = (int)(i - nvec * 4);
    out[i] = nz.sigma * (lane == 0 ? z[0] : lane == 1 ? z[1] : z[2]);
  }
}

// One element of the server step from Delta: MODE's update of x, m, v (no
// bias correction, as in the paper).
template <int MODE>
DEVINL void server_update(float delta, float& x, float& m, float& v, float lr,
                          float b1, float b2, float tau) {
  if constexpr (MODE == kServerMean) {
    x = x + delta;
  } else if constexpr (MODE == kServerAvgM) {
    m = fmaf(b1, m, delta);
    x = fmaf(lr, m, x);
  } else {
    m = fmaf(b1, m, (1.f - b1) * delta);
    if constexpr (MODE == kServerAdagrad) {
      v = fmaf(delta, delta, v);
    } else if constexpr (MODE == kServerAdam) {
      v = fmaf(b2, v, (1.f - b2) * delta * delta);
    } else {
      const float d2 = delta * delta;
      const float diff = v - d2;
      const float sign = (float)(diff > 0.f) - (float)(diff < 0.f);
      v = v - (1.f - b2) * d2 * sign;
    }
    x = fmaf(lr, m / (sqrtf(v) + tau), x);
  }
}

// x, m, v updated in place from the reduced D. round_state[2] == 0 is a
// uniform early exit: a skipped round writes nothing. Mean takes null m and
// v, AvgM null v. Without NOISE, Delta = fl(D * inv_W) and the pack is empty,
// so the kernel's arguments are what they always were; with NOISE the pack is
// one DpNoise, Delta = fl(D + fl(sigma * zeta)) and inv_W is never read.
template <int MODE, bool NOISE, typename... Noise>
__global__ void server_step_kernel(const float* __restrict__ D,
                                   float* __restrict__ x, float* __restrict__ m,
                                   float* __restrict__ v, long long n, float lr,
                                   float b1, float b2, float tau,
                                   const float* __restrict__ round_state,
                                   Noise... noise) {
  static_assert(sizeof...(Noise) == (NOISE ? 1 : 0), "one DpNoise iff NOISE");
  constexpr bool HAS_M = MODE != kServerMean;
  constexpr bool HAS_V = MODE >= kServerAdagrad;
  if (round_state[2] == 0.f) return;
  float inv_w = 0.f;
  DpNoise nz = {};
  if constexpr (NOISE) {
    nz = DpNoise{noise...};
  } else {
    inv_w = round_state[1];
  }
  const long long nvec = n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    const f32x4 dv = reinterpret_cast<const f32x4*>(D)[i];
    f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 mv = {}, vv = {};
    if constexpr (HAS_M) mv = reinterpret_cast<const f32x4*>(m)[i];
    if constexpr (HAS_V) vv = reinterpret_cast<const f32x4*>(v)[i];
    float z[4] = {};
    if constexpr (NOISE) unit_normals4(nz, (nz.elem_offset >> 2) + i, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xk = xv[k], mk = mv[k], vk = vv[k];
      const float delta = NOISE ? dv[k] + nz.sigma * z[k] : dv[k] * inv_w;
      server_update<MODE>(delta, xk, mk, vk, lr, b1, b2, tau);
      xv[k] = xk; mv[k] = mk; vv[k] = vk;
    }
    reinterpret_cast<f32x4*>(x)[i] = xv;
    if constexpr (HAS_M) reinterpret_cast<f32x4*>(m)[i] = mv;
    if constexpr (HAS_V) reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long long i = nvec * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float xk = x[i], mk = 0.f, vk = 0.f;
    if constexpr (HAS_M) mk = m[i];
    if constexpr (HAS_V) vk = v[i];
    float delta;
    if constexpr (NOISE) {
      float z[4];
      unit_normals4(nz, (nz.elem_offset >> 2) + nvec, z);
      const int lane = (int)(i - nvec * 4);
      delta = D[i] + nz.sigma * (lane == 0 ? z[0] : lane == 1 ? z[1] : z[2]);
    } else {
      delta = D[i] * inv_w;
    }
    server_update<MODE>(delta, xk, mk, vk, lr, b1, b2, tau);
    x[i] = xk;
    if constexpr (HAS_M) m[i] = mk;
    if constexpr (HAS_V) v[i] = vk;
  }
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

int launch_delta_sumsq(bool is_bf16, const void* theta, const float* x,
                       long long n, float* partials, hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(delta_sumsq_kernel<T>, dim3(grid), dim3(kBlock), 0, s,
                       (const T*)theta, x, n, partials);
  });
  return grid;
}

void launch_delta_scale_cast(bool is_bf16, float* dst, const void* theta,
                             const float* x, long long n, float alpha,
                             const float* clip_state, float* w_out,
                             hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_dtype(is_bf16, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(delta_scale_cast_kernel<T>, dim3(grid), dim3(kBlock), 0,
                       s, dst, (const T*)theta, x, n, alpha, clip_state, w_out);
  });
}

void launch_fedopt_finalize(const float* w_sum, float* round_state,
                            hipStream_t s) {
  hipLaunchKernelGGL(fedopt_finalize_kernel, dim3(1), dim3(1), 0, s, w_sum,
                     round_state);
}

// Host dispatch over the server optimizer: f(integral_constant<int, MODE>)
template <typename F>
static void dispatch_server_mode(int mode, F&& f) {
  switch (mode) {
    case kServerMean: f(std::integral_constant<int, kServerMean>{}); break;
    case kServerAvgM: f(std::integral_constant<int, kServerAvgM>{}); break;
    case kServerAdagrad: f(std::integral_constant<int, kServerAdagrad>{}); break;
    case kServerAdam: f(std::integral_constant<int, kServerAdam>{}); break;
    default: f(std::integral_constant<int, kServerYogi>{}); break;
  }
}

void launch_server_step(int mode, const float* D, float* x, float* m, float* v,
                        long long n, float lr, float b1, float b2, float tau,
                        const float* round_state, hipStream_t s) {
  const int grid = optim_grid(n);
  dispatch_server_mode(mode, [&](auto md) {
    hipLaunchKernelGGL((server_step_kernel<decltype(md)::value, false>),
                       dim3(grid), dim3(kBlock), 0, s, D, x, m, v, n, lr, b1,
                       b2, tau, round_state);
  });
}

static DpNoise dp_noise_args(unsigned long long seed, unsigned round,
                             unsigned stream, long long elem_offset,
                             float sigma) {
  return DpNoise{(unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32),
                 round, stream, elem_offset, sigma};
}

void launch_server_step_noise(int mode, const float* D, float* x, float* m,
                              float* v, long long n, float lr, float b1,
                              float b2, float tau, const float* round_state,
                              unsigned long long seed, unsigned round,
                              unsigned stream, long long elem_offset,
                              float sigma, hipStream_t s) {
  const int grid = optim_grid(n);
  const DpNoise nz = dp_noise_args(seed, round, stream, elem_offset, sigma);
  dispatch_server_mode(mode, [&](auto md) {
    hipLaunchKernelGGL((server_step_kernel<decltype(md)::value, true, DpNoise>),
                       dim3(grid), dim3(kBlock), 0, s, D, x, m, v, n, lr, b1,
                       b2, tau, round_state, nz);
  });
}

void launch_dp_noise(float* out, long long n, unsigned long long seed,
                     unsigned round, unsigned stream, long long elem_offset,
                     float sigma, hipStream_t s) {
  hipLaunchKernelGGL(dp_noise_kernel, dim3(optim_grid(n)), dim3(kBlock), 0, s,
                     out, n,
                     dp_noise_args(seed, round, stream, elem_offset, sigma));
}

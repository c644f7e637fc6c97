// Robust aggregation for the federated server step (gfx950): coordinate-wise
// median and trimmed mean over the clients' clipped updates (Yin et al.,
// "Byzantine-Robust Distributed Learning").
//
// Where the mean reduces sum_i w_i c_i d_i, these rules bring the K clients'
// unweighted rows u_i = c_i d_i to the root (U, K rows of n fp32) with their
// flags f_i. robust_finalize_kernel turns the flags into k live rows, the trim
// b = b_table[k] and round_state = [kept, 1 / kept, applied, skipped] in
// fedopt.hip's layout; robust_select_kernel<K> sorts the K values of every
// element in registers and writes the ascending sequential sum of
// s_b .. s_{k-b-1} to D, so that the unchanged server_step_kernel forms
// Delta = fl(D * round_state[1]). The definition is the docstring of
// fed/server_opt.py. Geometry as in fedopt.hip: optim_grid blocks of 256
// threads, 16 B per row per lane, scalar tail, grid-stride; nothing is read
// back by the host.
#include "common.h"

#include <utility>

// The kept sum is plain adds in ascending order: nothing may contract.
#pragma clang fp contract(off)

constexpr int kRobustMaxK = 16;

// One thread: flags[K] and the host-made b_table[K + 1] -> round_state and
// agg_state = [k, b]. b is clamped into [0, (k - 1) / 2], so kept >= 1
// whenever k >= 1 whatever the table holds. round_state[3] is only ever
// incremented here, on a round without a live row.
__global__ void robust_finalize_kernel(const float* __restrict__ flags,
                                       const int* __restrict__ b_table, int K,
                                       float* __restrict__ round_state,
                                       float* __restrict__ agg_state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int k = 0;
  for (int r = 0; r < K; ++r) k += flags[r] != 0.f ? 1 : 0;
  const bool applied = k > 0;
  int b = applied ? b_table[k] : 0;
  b = min(max(b, 0), applied ? (k - 1) / 2 : 0);
  const int kept = k - 2 * b;
  const float skipped = round_state[3];
  round_state[0] = (float)kept;
  round_state[1] = applied ? (float)(1.0 / (double)kept) : 0.f;
  round_state[2] = applied ? 1.f : 0.f;
  round_state[3] = applied ? skipped : skipped + 1.f;
  agg_state[0] = (float)k;
  agg_state[1] = (float)b;
}

// ---- the sorting network -----------------------------------------------------

// Batcher's merge exchange (Knuth, TAOCP 3, 5.2.2 Algorithm M) for any N: the
// compare-exchange pairs (a[c], b[c]), a < b, in order. 63 pairs at N = 16.
template <int N>
struct SortNet {
  int a[N * N / 2 + 1] = {};
  int b[N * N / 2 + 1] = {};
  int count = 0;
  constexpr SortNet() {
    int t = 0;
    while ((1 << t) < N) ++t;
    if (t == 0) return;
    for (int p = 1 << (t - 1); p > 0; p >>= 1) {
      int q = 1 << (t - 1), r = 0, d = p;
      while (true) {
        for (int i = 0; i + d < N; ++i)
          if ((i & p) == r) {
            a[count] = i;
            b[count] = i + d;
            ++count;
          }
        if (q == p) break;
        d = q - p;
        q >>= 1;
        r = p;
      }
    }
  }
};

template <int N>
struct SortNetHolder {
  static constexpr SortNet<N> net = SortNet<N>();
};
// Pair C of the network as plain constants (device code names no host object).
template <int N, size_t C>
constexpr int kSortLo = SortNetHolder<N>::net.a[C];
template <int N, size_t C>
constexpr int kSortHi = SortNetHolder<N>::net.b[C];
template <int N>
constexpr size_t kSortPairs = SortNetHolder<N>::net.count;

// Values are finite or +inf here (a dead row became +inf), so min / max is a
// permutation by value; -0.0 and +0.0 may leave in either order.
DEVINL void compare_exchange(float& lo, float& hi) {
  const float x = lo, y = hi;
  lo = __builtin_fminf(x, y);
  hi = __builtin_fmaxf(x, y);
}

// Every index below is a constant expression: v stays in registers.
template <int N, size_t... C>
DEVINL void sort_values(float (&v)[N], std::index_sequence<C...>) {
  (compare_exchange(v[kSortLo<N, C>], v[kSortHi<N, C>]), ...);
}

// The ascending sequential sum s_b + s_{b+1} + ... + s_{k-b-1} of the K
// values in v (dead rows already +inf, so the live ones sort to the front).
// The predicates are uniform; 0 + s_b is s_b by value.
template <int K>
DEVINL float kept_sum(float (&v)[K], int k, int b) {
  sort_values<K>(v, std::make_index_sequence<kSortPairs<K>>{});
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float next = acc + v[j];
    acc = (j >= b && j < k - b) ? next : acc;
  }
  return acc;
}

// D[e] = the kept sum of U[0 .. K)[e]. U's rows are `stride` elements apart
// (a multiple of 4, base 16-byte aligned). round_state[2] == 0 is a uniform
// early exit: a skipped round writes nothing. Every row is loaded, then a dead
// row's values are replaced by +inf with a select: no branch around a load.
// Hand-written loops (flat_walk's geometry): over the walker K = 13 takes 26
// more VGPRs and K >= 15 spills SGPRs.
template <int K>
__global__ void robust_select_kernel(float* __restrict__ D,
                                     const float* __restrict__ U,
                                     long long stride, long long n,
                                     const float* __restrict__ flags,
                                     const float* __restrict__ agg_state,
                                     const float* __restrict__ round_state) {
  if (round_state[2] == 0.f) return;
  const int k = (int)agg_state[0];
  const int b = (int)agg_state[1];
  bool live[K];
#pragma unroll
  for (int r = 0; r < K; ++r) live[r] = flags[r] != 0.f;
  const float inf = __builtin_inff();
  const long long nvec = n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long long)gridDim.x * blockDim.x) {
    f32x4 row[K];
#pragma unroll
    for (int r = 0; r < K; ++r)
      row[r] = reinterpret_cast<const f32x4*>(U + r * stride)[i];
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v[K];
#pragma unroll
      for (int r = 0; r < K; ++r) v[r] = live[r] ? row[r][c] : inf;
      o[c] = kept_sum<K>(v, k, b);
    }
    reinterpret_cast<f32x4*>(D)[i] = o;
  }
  for (long long i = nvec * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long long)gridDim.x * blockDim.x) {
    float v[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const float u = U[r * stride + i];
      v[r] = live[r] ? u : inf;
    }
    D[i] = kept_sum<K>(v, k, b);
  }
}

// ---- launchers -------------------------------------------------------------
#include "launchers.h"

void launch_robust_finalize(const float* flags, const int* b_table, int K,
                            float* round_state, float* agg_state,
                            hipStream_t s) {
  hipLaunchKernelGGL(robust_finalize_kernel, dim3(1), dim3(1), 0, s, flags,
                     b_table, K, round_state, agg_state);
}

template <int K>
static void launch_robust_select_k(int rows, int grid, float* D, const float* U,
                                   long long stride, long long n,
                                   const float* flags, const float* agg_state,
                                   const float* round_state, hipStream_t s) {
  if constexpr (K > kRobustMaxK) {
    return;                      // the binding refuses K outside 1 .. 16
  } else {
    if (rows == K)
      hipLaunchKernelGGL(robust_select_kernel<K>, dim3(grid), dim3(kBlock), 0, s,
                         D, U, stride, n, flags, agg_state, round_state);
    else
      launch_robust_select_k<K + 1>(rows, grid, D, U, stride, n, flags,
                                    agg_state, round_state, s);
  }
}

void launch_robust_select(int K, float* D, const float* U, long long stride,
                          long long n, const float* flags,
                          const float* agg_state, const float* round_state,
                          hipStream_t s) {
  launch_robust_select_k<1>(K, optim_grid(n), D, U, stride, n, flags, agg_state,
                            round_state, s);
}

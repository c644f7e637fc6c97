// Shared device helpers for the baton_amd gfx950 kernels.
//
// Written for CDNA4 (MI355X) only: 64-wide wavefronts, 256 CUs / 8 XCDs,
// HBM3E at ~8 TB/s. Every memory-bound kernel vectorizes to 16 B/lane
// (G13 in the CDNA HIP guide: hipcc does not auto-vectorize bf16 loads).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <type_traits>

#define DEVINL __device__ __forceinline__

constexpr int kWave = 64;           // CDNA wavefront width (not 32)
constexpr int kBlock = 256;         // default block: 4 waves
// Memory-bound grid cap: 256 CUs x 8 blocks, grid-stride the rest (G11).
constexpr int kMaxGrid = 2048;

static inline int elementwise_grid(long long n_vec, int block = kBlock) {
  long long b = (n_vec + block - 1) / block;
  if (b > kMaxGrid) b = kMaxGrid;
  if (b < 1) b = 1;
  return (int)b;
}

#include "gemm_strides.h"

// ---- dtype traits: 16-byte vectors ---------------------------------------

using bf16 = __hip_bfloat16;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct VecTraits;

template <>
struct VecTraits<float> {
  static constexpr int kElems = 4;  // 16 B
  using VecT = f32x4;
  DEVINL static void to_float(const VecT& v, float* out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = v[i];
  }
  DEVINL static void from_float(const float* in, VecT& v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = in[i];
  }
};

template <>
struct VecTraits<bf16> {
  static constexpr int kElems = 8;  // 16 B
  using VecT = s16x8;
  DEVINL static void to_float(const VecT& v, float* out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      unsigned int u = ((unsigned int)(unsigned short)v[i]) << 16;
      out[i] = __uint_as_float(u);
    }
  }
  DEVINL static void from_float(const float* in, VecT& v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // round-to-nearest-even f32 -> bf16
      unsigned int u = __float_as_uint(in[i]);
      unsigned int rounded = u + 0x7fff + ((u >> 16) & 1);
      v[i] = (short)(rounded >> 16);
    }
  }
};

DEVINL float bf16_to_f32(unsigned short h) {
  return __uint_as_float(((unsigned int)h) << 16);
}
DEVINL unsigned short f32_to_bf16(float f) {
  unsigned int u = __float_as_uint(f);
  unsigned int rounded = u + 0x7fff + ((u >> 16) & 1);
  return (unsigned short)(rounded >> 16);
}

// 16-B vector load/store to/from fp32 lanes (G13: hipcc does not
// auto-vectorize bf16 element loops)
template <typename T>
DEVINL void vload16(const T* p, float* f) {
  using VT = VecTraits<T>;
  typename VT::VecT v = *reinterpret_cast<const typename VT::VecT*>(p);
  VT::to_float(v, f);
}
template <typename T>
DEVINL void vstore16(T* p, const float* f) {
  using VT = VecTraits<T>;
  typename VT::VecT v;
  VT::from_float(f, v);
  *reinterpret_cast<typename VT::VecT*>(p) = v;
}

// Width-generic forms: W == 1 moves one element, any multiple of
// VecTraits<T>::kElems moves W / kElems 16-B vectors (the fp32 side buffers of
// a bf16 kernel: 8 lanes are two f32x4).
template <int W, typename T>
DEVINL void vload(const T* p, float* f) {
  if constexpr (W == 1) {
    f[0] = (float)p[0];
  } else {
    constexpr int E = VecTraits<T>::kElems;
    static_assert(W % E == 0, "W is 1 or whole 16-B vectors");
#pragma unroll
    for (int q = 0; q < W / E; ++q) vload16(p + q * E, f + q * E);
  }
}
template <int W, typename T>
DEVINL void vstore(T* p, const float* f) {
  if constexpr (W == 1) {
    p[0] = (T)f[0];
  } else {
    constexpr int E = VecTraits<T>::kElems;
    static_assert(W % E == 0, "W is 1 or whole 16-B vectors");
#pragma unroll
    for (int q = 0; q < W / E; ++q) vstore16(p + q * E, f + q * E);
  }
}

// W zeros (a fused zero fill)
template <int W, typename T>
DEVINL void vzero(T* p) {
  const float z[W] = {};
  vstore<W>(p, z);
}

// Row walker: the block's threads stride a row of C elements, as 16-B vectors
// when C % V == 0 (wave-uniform) and element by element otherwise. Calls
// body(element offset, integral_constant<int, W>) with W = V or 1.
template <typename T, typename F>
DEVINL void row_walk(int C, F&& body) {
  constexpr int V = VecTraits<T>::kElems;
  if ((C % V) == 0) {
    for (int cv = threadIdx.x; cv < C / V; cv += blockDim.x)
      body(cv * V, std::integral_constant<int, V>{});
  } else {
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      body(c, std::integral_constant<int, 1>{});
  }
}

// Flat walker of the streaming kernels: the grid strides n elements as
// vectors of V (thread t of the grid takes vectors t, t + threads, ...), then
// the n % V tail elements, one per thread. Calls body(element offset,
// integral_constant<int, W>) with W = V, then W = 1; a thread sees its
// elements in that order (the chained reductions depend on it). Launched on
// elementwise_grid blocks; the walker holds no arithmetic. The block size is
// read with the builtin: blockDim.x inside a device function keeps the
// non-uniform-block select and costs every kernel a load and ~20 instructions.
template <int V, typename F>
DEVINL void flat_walk(long long n, F&& body) {
  const long long block = __builtin_amdgcn_workgroup_size_x();  // blockDim.x
  const long long first = blockIdx.x * block + threadIdx.x;
  const long long step = gridDim.x * block;
  const long long nvec = n / V;
  for (long long i = first; i < nvec; i += step)
    body(i * V, std::integral_constant<int, V>{});
  for (long long i = nvec * V + first; i < n; i += step)
    body(i, std::integral_constant<int, 1>{});
}

// ---- per-sequence lengths (attention) ------------------------------------
// Last argument of a kernel with a VARLEN flag: its lengths (type L), or an
// empty struct so that the dense instantiations keep their code.
struct NoLens {};
template <bool VARLEN, typename L>
using LenArg = std::conditional_t<VARLEN, L, NoLens>;
// clamped into [0, S]: a bad length cannot move an access out of bounds
DEVINL int clamp_len(int len, int S) { return min(max(len, 0), S); }

// Host dispatch over two template flags: f(bool_constant<a>, bool_constant<b>)
template <typename F>
void dispatch2(bool a, bool b, F&& f) {
  auto on_a = [&](auto A) {
    if (b) f(A, std::true_type{}); else f(A, std::false_type{});
  };
  if (a) on_a(std::true_type{}); else on_a(std::false_type{});
}

// Host dispatch over the element type: f(TypeTag<bf16>) or f(TypeTag<float>)
template <typename T>
struct TypeTag { using type = T; };
template <typename F>
void dispatch_dtype(bool is_bf16, F&& f) {
  if (is_bf16) f(TypeTag<bf16>{}); else f(TypeTag<float>{});
}

// ---- reductions ----------------------------------------------------------

DEVINL float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;  // valid in lane 0 of the wave
}

DEVINL float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, kWave));
  return v;
}

// Block-level sum reduction; returns the total in every thread.
// Requires a __shared__ float scratch[block/kWave] from the caller.
DEVINL float block_reduce_sum(float v, float* scratch) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int nwaves = blockDim.x / kWave;
  v = wave_reduce_sum(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float total = 0.f;
#pragma unroll 4
  for (int i = 0; i < nwaves; ++i) total += scratch[i];
  __syncthreads();
  return total;
}

// ---- GEMM block id -------------------------------------------------------
// Linear id of this block in its (x, y) grid; tile_n = id % gridDim.x,
// tile_m = id / gridDim.x. XCD-aware remap (T1): the dispatcher places
// block b on XCD b%8, so consecutive ids (which share an operand panel)
// would land on different per-XCD L2s; give each XCD a contiguous chunk
// instead (bijective form).
DEVINL int xcd_block_id(int use_swz) {
  const int nwg = gridDim.x * gridDim.y;
  int bid = blockIdx.y * gridDim.x + blockIdx.x;
  if (use_swz && nwg >= 64) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  return bid;
}

// ---- canonical K-slice LDS image (shared by gemm.hip / conv.hip) ---------
// bf16: LINEAR 64-B rows (32 elements) with a 16-B slot XOR swizzle —
// compatible with global_load_lds (lane-linear dest) and bank-conflict-free
// for both ds_read_b128 fragment groups and transposed scalar writes
// (contiguous k elements spread banks naturally).
// f32: padded rows (+2 elements) with scalar b32 fragment reads.
constexpr int kBKElems = 32;   // K-slice width in elements

template <typename T>
constexpr int lds_row_elems() {
  return sizeof(T) == 2 ? kBKElems : kBKElems + 2;
}

template <typename T>
DEVINL int lds_off(int row, int col) {
  if constexpr (sizeof(T) == 2) {
    const int sl = col >> 3;
    return row * kBKElems + ((sl ^ ((row >> 2) & 3)) << 3) + (col & 7);
  } else {
    return row * (kBKElems + 2) + col;
  }
}

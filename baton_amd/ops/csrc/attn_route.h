// Host-side router of the attention family: which views the flash kernels
// accept, their grids and LDS sizes, and which softmax kernel, vector form and
// grid a row problem gets. Pure (no HIP, no torch, no environment), like
// gemm_plan.h, conv_route.h and norm_route.h, so every gate can be checked
// without a GPU; flash.hip sizes its LDS from the functions below, the
// launchers launch what a route names and bindings.cpp refuses from its text.
#pragma once
#include <string>

// ---- flash attention -------------------------------------------------------
namespace fa {
constexpr int THREADS = 256;     // 4 waves
constexpr int QW = 32;           // q rows per wave
constexpr int QB = 128;          // q rows per block (fwd, dq)
constexpr int KVB = 64;          // kv tile (fwd, dq)
constexpr int KVBB = 128;        // kv rows per block (dkv), 32 per wave
constexpr int DELTA_ROWS = 4;    // rows per block of the delta kernel

// LDS bytes per kernel (2 per bf16). fwd: K rows and V^T, double-buffered;
// dq: K rows | V rows | K^T; dkv: K, V rows | Q, dO [32][dh] | Q^T, dO^T
constexpr unsigned fwd_lds_bytes(int dh) { return 2u * (4 * KVB * dh); }
constexpr unsigned dq_lds_bytes(int dh) { return 2u * (3 * KVB * dh); }
constexpr unsigned dkv_lds_bytes(int dh) {
  return 2u * (2 * KVBB * dh + 4 * 32 * dh);
}
}  // namespace fa

// One [B, S, heads, dh] view. The kernels move 16-byte vectors at element
// offsets that are multiples of 8 from (batch, seq, head) row starts, so dh
// must be contiguous and the base and outer strides keep them aligned.
struct AttnView {
  bool bf16;
  long long sB, sS, sH;   // outer strides in elements
  long long sD;           // stride(3)
  int base_mod16;         // base address % 16
};

// q, k, v, o for the forward, all eight for the backward, q, k, v alone
// for _flash_eligible
enum FlashViewId { kQ, kK, kV, kO, kDout, kDq, kDk, kDv, kFlashMaxViews };
constexpr const char* kFlashViewName[kFlashMaxViews] = {
    "q", "k", "v", "o", "dout", "dq", "dk", "dv"};

struct FlashProblem {
  int B, S, H, KVH, DH;
  bool causal, varlen;
  int nviews;
  AttnView view[kFlashMaxViews];
};

struct FlashRoute {
  bool eligible;
  std::string refusal;    // names the argument; empty when eligible
  int G;                  // q heads per kv head
  int grid_fwd[2], grid_delta[2], grid_dq[2], grid_dkv[2];   // (x, y)
  unsigned lds_fwd, lds_dq, lds_dkv;
};

inline FlashRoute flash_route(const FlashProblem& p) {
  FlashRoute rt{};
  auto refuse = [&](const std::string& why) { return rt.refusal = why, rt; };
  for (int i = 0; i < p.nviews; ++i) {
    const AttnView& t = p.view[i];
    const std::string name = kFlashViewName[i];
    if (!t.bf16) return refuse(name + " must be a bf16 GPU tensor");
    if (t.sD != 1) return refuse(name + " head_dim must be contiguous");
    if (t.base_mod16 != 0)
      return refuse(name + " must start on a 16-byte boundary");
    if (t.sB % 8 != 0 || t.sS % 8 != 0 || t.sH % 8 != 0)
      return refuse(name +
                    " strides must be multiples of 8 elements (16 bytes)");
  }
  if (p.DH != 32 && p.DH != 64 && p.DH != 128)
    return refuse("flash: unsupported head_dim " + std::to_string(p.DH));
  if (p.KVH <= 0 || p.H % p.KVH != 0)
    return refuse("q heads must be a multiple of kv heads");
  rt.eligible = true;
  rt.G = p.H / p.KVH;
  rt.grid_fwd[0] = rt.grid_dq[0] = (p.S + fa::QB - 1) / fa::QB;
  rt.grid_dkv[0] = (p.S + fa::KVBB - 1) / fa::KVBB;
  rt.grid_delta[0] = (p.S + fa::DELTA_ROWS - 1) / fa::DELTA_ROWS;
  for (int* g : {rt.grid_fwd, rt.grid_delta, rt.grid_dq, rt.grid_dkv})
    g[1] = p.B * p.H;
  rt.lds_fwd = fa::fwd_lds_bytes(p.DH);
  rt.lds_dq = fa::dq_lds_bytes(p.DH);
  rt.lds_dkv = fa::dkv_lds_bytes(p.DH);
  return rt;
}

// ---- row softmax over [R, C] -------------------------------------------------
constexpr int kSoftmaxMaxGrid = 2048;  // blocks; grid-stride past it
constexpr int kSoftmaxWaveMaxC = 1024; // up to here: one wave per row
constexpr int kSoftmaxWaveRows = 4;    // rows per block of the wave kernels
// vectors need enough of them to keep a wave busy: at C = 128 they left 16
// of 256 threads active and measured SLOWER than scalar
constexpr int kSoftmaxVecMinVecs = 64;

constexpr bool softmax_vec(int C, int V) {
  return (C % V) == 0 && C >= V * kSoftmaxVecMinVecs;
}

struct SoftmaxRoute {
  bool wave;            // wave-per-row kernel, else row-per-block
  bool vec;             // 16-byte vectors, else element by element
  int rows_per_block;   // 4 (wave) or 1 (block)
  int grid;             // min(kSoftmaxMaxGrid, ceil(R / rows_per_block))
  bool capped;          // more row blocks than the grid: a second trip
};

inline SoftmaxRoute softmax_route(long long R, int C, bool bf16) {
  SoftmaxRoute rt{};
  rt.wave = C <= kSoftmaxWaveMaxC;
  rt.vec = softmax_vec(C, bf16 ? 8 : 4);
  rt.rows_per_block = rt.wave ? kSoftmaxWaveRows : 1;
  const long long blocks = (R + rt.rows_per_block - 1) / rt.rows_per_block;
  rt.capped = blocks > kSoftmaxMaxGrid;
  rt.grid = rt.capped ? kSoftmaxMaxGrid : (int)blocks;
  return rt;
}

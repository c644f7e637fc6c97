// Pixel-major tap-shared 3x3 stride-1 pad-1 wgrad (gfx950, bf16):
//   dw[co][tap][ci] += sum_px dy[px][co] * x[px + tap][ci]
// fp32 out, K = pixels split over grid.z into fp32 atomics.
//
// Both operands keep the layout they have in HBM ([pixel][channel], NHWC)
// all the way into LDS: every staged piece is a straight 16-B
// global_load_lds (destination lane-linear, source chosen per lane, a 16-B
// zero page for window positions outside the image), and the MFMA
// fragments come out of ds_read_b64_tr_b16, which transposes [px][ch]
// rows into the k-contiguous operand on the way to the registers. So dy
// needs no [Cout][P] copy, and because a tap is a whole-row shift in a
// pixel-major image, ONE halo'd x window per k-step serves all 9 taps: a
// tap is the `offset:` immediate of the read.
//
// Block: 512 threads, 8 waves as 2 (co) x 4 (ci); tile 64 co x 9 taps x
// 64 ci (72 accumulator VGPRs per lane); 32 pixels per k-step. Per k-step
// a wave issues 4 A reads + 18 B reads for 18 MFMAs.
//
// LDS image, window layout, k order and the bank argument (every
// transposed read conflict-free: degree 1) are in wgrad_px_map.h; this
// file calls those functions and keeps no copy of the maps.
//
// Pipeline: NBUF = 3 buffers, two k-steps of glds in flight. Every wave
// issues exactly PASSES glds per staged step and nothing else touches
// vmcnt inside the loop, so at the top of step kt `s_waitcnt
// vmcnt(PASSES)` leaves exactly step kt+1's pieces outstanding (vmcnt(0)
// on the last step, when nothing younger is in flight - a count larger
// than what is in flight would not drain). The raw s_barrier after it
// makes step kt's buffer visible to all waves and, since every wave has
// passed step kt-1's reads, frees that buffer for step kt+2's glds.
#include "common.h"
#include "wgrad_px_map.h"

namespace wgpx {

typedef short s16x4 __attribute__((ext_vector_type(4)));
#define WGPX_LDS __attribute__((address_space(3)))

__device__ __align__(16) const unsigned int g_zero16[4] = {0, 0, 0, 0};

// One transposed read. Inline asm, not the builtin: the compiler orders a
// builtin LDS read behind EVERY outstanding global_load_lds (vmcnt(0)),
// which would drain the two k-steps kept in flight. The price is that the
// lgkmcnt waits are ours too (lgkm_wait ties them to the registers the
// MFMAs consume, so they cannot be scheduled past the wait).
template <int OFF>
DEVINL s16x4 tr_read(unsigned addr) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
template <int N>
DEVINL void lgkm_wait(s16x4& a, s16x4& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
DEVINL s16x8 cat(s16x4 lo, s16x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int W>
__global__ __launch_bounds__(THREADS, 4) void wgrad_px_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ dw, int H, int Cin, int Cout, long long steps,
    int sps) {
  // the only LDS object: dynamic, 16-B aligned base (transposed reads need
  // 8-B aligned lane addresses; every offset below is a multiple of 8)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int PASSES = passes_of(W);
  constexpr int BUFB = PASSES * THREADS * 16;

  const Geom g = make_geom(H, W);
  const long long s0 = (long long)blockIdx.z * sps;
  const long long left = steps - s0;
  const int nk = (int)(left < sps ? left : sps);
  if (nk <= 0) return;                       // block-uniform
  const int ci0 = blockIdx.x * TILE, co0 = blockIdx.y * TILE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wid >> 2) * 32;           // co half
  const int wn0 = (wid & 3) * 16;            // ci quarter

  // ---- staging state: one source per (pass, thread) --------------------
  const long long p0 = s0 * PXK;
  int h0 = (int)((p0 / W) % H);              // image row of the step's 1st px
  const bf16* src[PASSES];
  long long stride[PASSES];
  int kind[PASSES], hrel[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const ChunkSrc cs = chunk_src(g, p * THREADS + tid);
    kind[p] = cs.kind;
    hrel[p] = cs.hrel;
    if (cs.kind == 1) {
      src[p] = dy + (p0 + cs.rel) * Cout + co0 + cs.sub * 8;
      stride[p] = (long long)PXK * Cout;
    } else if (cs.kind == 2) {
      // may point outside x while its row is invalid; never loaded then
      src[p] = x + (p0 + cs.rel) * Cin + ci0 + cs.sub * 8;
      stride[p] = (long long)PXK * Cin;
    } else {
      src[p] = (const bf16*)g_zero16;
      stride[p] = 0;
    }
  }
  auto stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const bool ok =
          kind[p] == 1 || (kind[p] == 2 && x_row_valid(g, h0, hrel[p]));
      const bf16* s = ok ? src[p] : (const bf16*)g_zero16;
      auto gp = (const __attribute__((address_space(1))) unsigned int*)s;
      auto lp = (WGPX_LDS unsigned int*)(lds + buf * BUFB +
                                         (p * THREADS + wid * 64) * 16);
      __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
      src[p] += stride[p];
    }
    h0 += g.R;
    while (h0 >= H) h0 -= H;
  };

  // ---- fragment addresses ----------------------------------------------
  const int a0 = a_read_addr(lane, 0) + wm0 * 2;
  const int a1 = a_read_addr(lane, 1) + wm0 * 2;
  const int b0 = b_read_addr(g, lane, 0) + wn0 * 2;
  const int b1 = b_read_addr(g, lane, 1) + wn0 * 2;

  const unsigned lds_base = (unsigned)(size_t)(WGPX_LDS unsigned char*)lds;

  f32x4 acc[2][9] = {};

  stage(0);
  if (nk > 1) stage(1);
  int cur = 0, nxt = 2;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PASSES) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) stage(nxt);

    // 4 A reads + 18 B reads, B two taps ahead of the MFMAs. LDS reads
    // return in order, so lgkmcnt(4) means all but the 2 newest taps landed.
    const unsigned ab = lds_base + cur * BUFB;
    s16x4 al0 = tr_read<0>(ab + a0), ah0 = tr_read<0>(ab + a1);
    s16x4 al1 = tr_read<32>(ab + a0), ah1 = tr_read<32>(ab + a1);
    s16x4 bl[9], bh[9];
#define WGPX_RD(t)                                                  \
  bl[t] = tr_read<tap_bytes(W, (t) / 3, (t) % 3)>(ab + b0);         \
  bh[t] = tr_read<tap_bytes(W, (t) / 3, (t) % 3)>(ab + b1);
#define WGPX_MM(t, n)                                               \
  {                                                                 \
    lgkm_wait<n>(bl[t], bh[t]);                                     \
    const s16x8 bf = cat(bl[t], bh[t]);                             \
    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(            \
        a_frag0, bf, acc[0][t], 0, 0, 0);                           \
    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(            \
        a_frag1, bf, acc[1][t], 0, 0, 0);                           \
  }
    WGPX_RD(0) WGPX_RD(1) WGPX_RD(2)
    lgkm_wait<4>(al0, ah0);
    lgkm_wait<4>(al1, ah1);
    const s16x8 a_frag0 = cat(al0, ah0), a_frag1 = cat(al1, ah1);
    WGPX_MM(0, 4) WGPX_RD(3)
    WGPX_MM(1, 4) WGPX_RD(4)
    WGPX_MM(2, 4) WGPX_RD(5)
    WGPX_MM(3, 4) WGPX_RD(6)
    WGPX_MM(4, 4) WGPX_RD(7)
    WGPX_MM(5, 4) WGPX_RD(8)
    WGPX_MM(6, 4)
    WGPX_MM(7, 2)
    WGPX_MM(8, 0)
#undef WGPX_RD
#undef WGPX_MM
    cur = cur + 1 == NBUF ? 0 : cur + 1;
    nxt = nxt + 1 == NBUF ? 0 : nxt + 1;
  }

  const int col_in_frag = lane & 15, row_base = (lane >> 4) * 4;
  const long long ldw = 9LL * Cin;
#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = co0 + wm0 + mf * 16 + row_base + r;
        const long long col = (long long)t * Cin + ci0 + wn0 + col_in_frag;
        if (gridDim.z == 1)
          dw[row * ldw + col] = acc[mf][t][r];
        else
          atomicAdd(&dw[row * ldw + col], acc[mf][t][r]);
      }
}

// steps = k-steps in all, sps = k-steps per grid.z slice (from the route)
template <int W>
static void launch_w(const bf16* dy, const bf16* x, float* dw, int H, int Cin,
                     int Cout, long long steps, int sps, dim3 grid,
                     hipStream_t s) {
  constexpr int smem = NBUF * passes_of(W) * THREADS * 16;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)wgrad_px_kernel<W>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              smem);
    attr_set = true;
  }
  hipLaunchKernelGGL(wgrad_px_kernel<W>, grid, dim3(THREADS), smem, s, dy, x,
                     dw, H, Cin, Cout, steps, sps);
}

}  // namespace wgpx

#include "launchers.h"

// dw (fp32, zero-initialised by the caller) += wgrad of a 3x3 stride-1
// pad-1 conv, dy in its natural [P][Cout] layout. What the kernel can run
// is wgpx::eligible() - bf16, Cin % 64 == 0, Cout % 64 == 0, W in {4, 8, 16,
// 32}, H >= 4, and with R = 32 / W rows per k-step H % R == 0 (or R % H == 0
// when H < R), N*H*W % 32 == 0 - and the route's slices must tile the
// k-steps. Returns false, launching nothing, otherwise.
bool launch_conv_wgrad_px(const ConvRoute& rt, const ConvProblem& p,
                          const void* dy, const void* x, void* dw,
                          hipStream_t s) {
  using namespace wgpx;
  if (rt.kind != ConvKind::WgradPx || !conv_wgrad_px_fits(p)) return false;
  const long long steps = (long long)p.N * p.H * p.W / PXK;
  const long long sps = rt.p_chunk / PXK;
  if (rt.bm != TILE || rt.bn != TILE || rt.grid_x != p.Cin / TILE ||
      rt.grid_y != p.Cout / TILE || rt.splits < 1 || rt.grid_z != rt.splits ||
      sps < 1 || rt.p_chunk % PXK != 0 || sps > (1 << 30) ||
      rt.splits * sps < steps || (rt.splits - 1) * sps >= steps)
    return false;
  auto dyp = (const bf16*)dy;
  auto xp = (const bf16*)x;
  auto dwp = (float*)dw;
  const dim3 grid(rt.grid_x, rt.grid_y, rt.splits);
  const int H = p.H, Cin = p.Cin, Cout = p.Cout, k = (int)sps;
  switch (p.W) {
    case 4: launch_w<4>(dyp, xp, dwp, H, Cin, Cout, steps, k, grid, s); break;
    case 8: launch_w<8>(dyp, xp, dwp, H, Cin, Cout, steps, k, grid, s); break;
    case 16: launch_w<16>(dyp, xp, dwp, H, Cin, Cout, steps, k, grid, s); break;
    default: launch_w<32>(dyp, xp, dwp, H, Cin, Cout, steps, k, grid, s); break;
  }
  return true;
}

// Fused flash attention (gfx950, bf16): forward + backward.
//
// Replaces the materialized S x S score path (batched GEMMs + standalone
// softmax in attention.hip) for the transformer configs: per Q-tile the
// kernel walks K/V tiles with an online softmax, so scores never touch HBM
// and the softmax/transpose/dP round-trips disappear from the profile
// (reference computation: torch softmax(QK^T)V inside
// nn.MultiheadAttention-equivalents; this serves the BERT/Llama BASELINE
// configs).
//
// Structure (CDNA4 guide §B "fused attention prefill" recipe, adapted):
//   * workgroup = 4 waves x 32 q rows = 128 q rows of one (batch, q-head);
//   * swapped QK^T: S^T = mfma(A=K, B=Q^T) per 32x32x16 — BOTH fragments
//     are contiguous row-major 16-B reads, and the q row is LANE-local
//     (col j = lane&31), so the whole online softmax runs in registers:
//     per-row state (m, l) is one scalar per lane, the row max needs one
//     __shfl_xor(32) to merge the two half-waves;
//   * P -> bf16 B-fragments via float2-to-bf16x2 packs + permlane32_swap
//     (guide T12): the half-waves hold complementary kv quads, one swap
//     per dword pair rebuilds the mfma fragment layout;
//   * PV accumulates O^T = mfma(A=V^T, B=P^T): V is staged TRANSPOSED into
//     LDS ([dh][kv] image) so the A-fragment read is again a contiguous
//     16-B row read; O^T keeps q lane-local, so the online rescale
//     o *= alpha is a lane-local scalar multiply;
//   * K and V^T LDS images are 16-B-slot XOR-swizzled (guide T2 / G4):
//     the fragment reads walk rows per lane at a fixed column slot, which
//     is the 8-16-way-conflict pattern on power-of-2 row strides;
//   * K/V staging is double-buffered with the async-STAGE split (T14):
//     next tile's global loads issue before the compute phase, the LDS
//     write lands after the barrier.
//
// Backward (two-pass recompute, FlashAttention-2 style, no fp32 atomics):
//   * a tiny delta kernel: delta[q] = rowsum(dO o O);
//   * dQ kernel (q-tile-major, same geometry as forward): recomputes
//     P^T = exp(scale*S^T - lse), dP^T = mfma(A=V, B=dO^T-frags),
//     dS^T = P^T o (dP^T - delta) * scale, dQ^T += mfma(A=K^T, B=dS^T);
//   * dK/dV kernel (kv-tile-major, each wave owns 32 kv rows): S/P/dP in
//     the mirrored orientation (kv lane-local), dV^T += mfma(A=dO^T, B=P),
//     dK^T += mfma(A=Q^T, B=dS) with Q/dO staged row-major AND transposed.
// Tile sizes, grids and LDS sizes are attn_route.h's.
#include <stdexcept>

#include "common.h"
#include "launchers.h"

namespace fa {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// pack two f32 into one dword of 2 bf16 (compiler emits v_cvt_pk_bf16_f32)
DEVINL unsigned int pk_bf16(float lo, float hi) {
  __hip_bfloat162 t = __float22bfloat162_rn(float2{lo, hi});
  return *reinterpret_cast<unsigned int*>(&t);
}

// eight consecutive fp32 -> one bf16 MFMA fragment (T12 half-swap)
DEVINL s16x8 pack_frag(const float* p) {
  unsigned int A = pk_bf16(p[0], p[1]);
  unsigned int B = pk_bf16(p[2], p[3]);
  unsigned int C = pk_bf16(p[4], p[5]);
  unsigned int D = pk_bf16(p[6], p[7]);
  {
    u32x2 r = __builtin_amdgcn_permlane32_swap(A, C, false, false);
    A = r[0]; C = r[1];
  }
  {
    u32x2 r = __builtin_amdgcn_permlane32_swap(B, D, false, false);
    B = r[0]; D = r[1];
  }
  unsigned int dw[4] = {A, B, C, D};
  return *reinterpret_cast<const s16x8*>(dw);
}

// K image: [KVB][DH] with 16-B slot XOR (row stride is power of two; the
// fragment read is row-per-lane at a fixed slot -> up to 16-way without it)
template <int DH>
DEVINL int koff(int kv, int d) {
  constexpr int XM = (DH / 8 > 16 ? 16 : DH / 8) - 1;
  return kv * DH + ((((d >> 3) ^ kv) & XM) << 3) + (d & 7);
}
// V^T image: [DH][KVB], same treatment (rows are d, cols are kv)
DEVINL int voff(int d, int kv) {
  return d * KVB + ((((kv >> 3) ^ d) & 7) << 3) + (kv & 7);
}
// Q^T / dO^T images of dk/dv: [DH][32] (rows are d, cols are q)
DEVINL int qtoff(int d, int q) {
  return d * 32 + ((((q >> 3) ^ d) & 3) << 3) + (q & 7);
}

DEVINL s16x8 lds128(const bf16* p) {
  return *reinterpret_cast<const __attribute__((address_space(3)))
             s16x8*>((const __attribute__((address_space(3))) bf16*)p);
}
DEVINL void lds_store128(bf16* p, s16x8 v) {
  *reinterpret_cast<__attribute__((address_space(3))) s16x8*>(
      (__attribute__((address_space(3))) bf16*)p) = v;
}

// 16-byte chunk idx of a [rows][DH] tile: its tile row and 8-element slot
template <int DH> DEVINL int chunk_row(int idx) { return idx / (DH / 8); }
template <int DH> DEVINL int chunk_slot(int idx) { return idx % (DH / 8); }

// that chunk of two operands (row strides lda, ldb) whose tile starts at
// global row r0; zero from global row L on
template <int DH>
DEVINL void load_chunk2(int idx, int r0, int L, const bf16* A, long long lda,
                        const bf16* B, long long ldb, s16x8& a, s16x8& b) {
  const int g = r0 + chunk_row<DH>(idx);
  const int slot = chunk_slot<DH>(idx);
  if (g < L) {
    a = *reinterpret_cast<const s16x8*>(&A[(long long)g * lda + slot * 8]);
    b = *reinterpret_cast<const s16x8*>(&B[(long long)g * ldb + slot * 8]);
  } else {
    a = s16x8{};
    b = s16x8{};
  }
}

// ---- per-sequence lengths ---------------------------------------------------
//
// VARLEN instantiations take seq_lens (int32 [B], right padding: the live
// tokens of batch element b are rows 0 .. L_b - 1) as their last argument and
// run "the same kernel at S = L_b": L replaces S in every row guard, key mask
// and loop bound, so the live rows walk the same tiles in the same order as
// the dense kernel on the [:L_b] slices and are bit-identical to it. Rows
// L_b .. S-1 of every output are stored as +0; nothing is read from them.
// The dense instantiations take an empty struct instead and keep their code.
template <bool VARLEN> using Lens = LenArg<VARLEN, const int*>;

// block-uniform (b comes from blockIdx): stays in an SGPR. Clamped into
// [0, S] so a bad length cannot move an access out of bounds.
template <bool VARLEN>
DEVINL int live_len(Lens<VARLEN> lens, int b, int S) {
  if constexpr (VARLEN) return clamp_len(lens[b], S);
  else return S;
}

// one lane's share of a [.., DH] output row (the epilogues' store pattern):
// 4-element run qd of 32-column block db starts at this element
DEVINL int run_off(int db, int qd, int hi) { return db * 32 + qd * 8 + hi * 4; }

template <int DH>
DEVINL void store_zero_row(bf16* row, int hi) {
#pragma unroll
  for (int db = 0; db < DH / 32; ++db)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
      *reinterpret_cast<u32x2*>(&row[run_off(db, qd, hi)]) = u32x2{0u, 0u};
}

// the accumulators' row, stored as bf16; SCALED (compile time, so the others
// keep their code) multiplies by mul first: the forward's 1 / l
template <int DH, bool SCALED = false>
DEVINL void store_row(bf16* row, const f32x16* acc, int hi, float mul = 1.f) {
#pragma unroll
  for (int db = 0; db < DH / 32; ++db)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      unsigned int w0, w1;
      if constexpr (SCALED) {
        w0 = pk_bf16(acc[db][qd * 4 + 0] * mul, acc[db][qd * 4 + 1] * mul);
        w1 = pk_bf16(acc[db][qd * 4 + 2] * mul, acc[db][qd * 4 + 3] * mul);
      } else {
        w0 = pk_bf16(acc[db][qd * 4 + 0], acc[db][qd * 4 + 1]);
        w1 = pk_bf16(acc[db][qd * 4 + 2], acc[db][qd * 4 + 3]);
      }
      *reinterpret_cast<u32x2*>(&row[run_off(db, qd, hi)]) = u32x2{w0, w1};
    }
}

// ---- forward ---------------------------------------------------------------
//
// grid: (ceil(S/QB), B*H). q/k/v strided [B,S,(kv)h,DH]; o [B,S,H,DH]
// (d contiguous); lse [B*H, S] fp32 = m + log(l).
template <int DH, bool CAUSAL, bool VARLEN>
__global__ __launch_bounds__(THREADS) void flash_fwd_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O,
    float* __restrict__ LSE, int S, int H, int G, float scale,
    long long sqB, long long sqS, long long sqH,
    long long skB, long long skS, long long skH,
    long long svB, long long svS, long long svH,
    long long soB, long long soS, long long soH,
    Lens<VARLEN> lens) {
  constexpr int F = DH / 16;        // QK^T mfma count per 32-kv subtile
  constexpr int DB = DH / 32;       // O^T 32-row blocks
  constexpr int NCK = DH / 32;      // 16-B staging chunks per thread/operand

  __shared__ bf16 lds[fwd_lds_bytes(DH) / sizeof(bf16)];
  auto kbuf = [&](int b) -> bf16* { return lds + b * KVB * DH; };
  auto vbuf = [&](int b) -> bf16* { return lds + 2 * KVB * DH + b * DH * KVB; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;

  const int qblk = blockIdx.x;
  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int kvh = h / G;

  const bf16* Qp = Q + b * sqB + h * sqH;
  const bf16* Kp = K + b * skB + kvh * skH;
  const bf16* Vp = V + b * svB + kvh * svH;
  bf16* Op = O + b * soB + h * soH;

  const int q0 = qblk * QB;
  const int qg = q0 + wid * QW + lq;          // this lane's q row
  const int L = live_len<VARLEN>(lens, b, S);
  if (VARLEN && q0 >= L) {
    // dead block (taken by the whole block, before any barrier): no loads
    if (qg < S) {
      if (lane < 32) LSE[(long long)bh * S + qg] = 0.f;
      store_zero_row<DH>(Op + (long long)qg * soS, hi);
    }
    return;
  }
  const bool qvalid = qg < L;
  const int qmax_w = min(q0 + wid * QW + QW - 1, L - 1);

  // Q^T B-fragments: lane holds Q[qg][f*16 + hi*8 .. +7]
  s16x8 qf[F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    if (qvalid)
      qf[f] = *reinterpret_cast<const s16x8*>(
          &Qp[(long long)qg * sqS + f * 16 + hi * 8]);
    else
      qf[f] = s16x8{};
  }

  f32x16 o_acc[DB] = {};
  float m_run = -INFINITY;
  float l_run = 0.f;

  const int nkv_block = CAUSAL ? min(L, q0 + QB) : L;
  const int ntile = (nkv_block + KVB - 1) / KVB;

  // ---- staging helpers (register-staged; T14 split) ----
  s16x8 kreg[NCK], vreg[NCK];
  auto stage_load = [&](int t) {
#pragma unroll
    for (int c = 0; c < NCK; ++c)
      load_chunk2<DH>(c * THREADS + tid, t * KVB, L, Kp, skS, Vp, svS,
                      kreg[c], vreg[c]);
  };
  auto stage_write = [&](int buf) {
    bf16* kb = kbuf(buf);
    bf16* vb = vbuf(buf);
#pragma unroll
    for (int c = 0; c < NCK; ++c) {
      const int kv = chunk_row<DH>(c * THREADS + tid);
      const int slot = chunk_slot<DH>(c * THREADS + tid);
      lds_store128(&kb[koff<DH>(kv, slot * 8)], kreg[c]);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vb[voff(slot * 8 + j, kv)] = ((const bf16*)&vreg[c])[j];
    }
  };

  stage_load(0);
  stage_write(0);
  __syncthreads();

  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1;
    const int k0 = t * KVB;
    if (t + 1 < ntile) stage_load(t + 1);   // issue early (T14)

    const bool active = !CAUSAL || k0 <= qmax_w;
    float p0[16], p1[16];
    if (active) {
      const bf16* kb = kbuf(cur);
      f32x16 sa0 = {}, sa1 = {};
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const s16x8 a0 = lds128(&kb[koff<DH>(lq, f * 16 + hi * 8)]);
        const s16x8 a1 = lds128(&kb[koff<DH>(32 + lq, f * 16 + hi * 8)]);
        sa0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[f], sa0, 0, 0, 0);
        sa1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[f], sa1, 0, 0, 0);
      }
      // mask + scale
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kvl = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int kv_g0 = k0 + kvl;
        const int kv_g1 = k0 + 32 + kvl;
        const bool v0 = kv_g0 < L && (!CAUSAL || kv_g0 <= qg);
        const bool v1 = kv_g1 < L && (!CAUSAL || kv_g1 <= qg);
        p0[r] = v0 ? sa0[r] * scale : -1e30f;
        p1[r] = v1 ? sa1[r] * scale : -1e30f;
        tm = fmaxf(tm, fmaxf(p0[r], p1[r]));
      }
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      const float mn = fmaxf(m_run, tm);
      const float alpha = __expf(m_run - mn);
      m_run = mn;
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p0[r] = __expf(p0[r] - mn);
        p1[r] = __expf(p1[r] - mn);
        rs += p0[r] + p1[r];
      }
      l_run = l_run * alpha + rs + __shfl_xor(rs, 32, 64);
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;

      // P -> bf16 fragments; frag[st][halfk]
      s16x8 pf[2][2];
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const float* p = st == 0 ? p0 : p1;
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) pf[st][hk] = pack_frag(p + hk * 8);
      }
      // PV: O^T += V^T-frag x P-frag
      const bf16* vbp = vbuf(cur);
#pragma unroll
      for (int db = 0; db < DB; ++db) {
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int hk = 0; hk < 2; ++hk) {
            const s16x8 av = lds128(
                &vbp[voff(db * 32 + lq, st * 32 + hk * 16 + hi * 8)]);
            o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                av, pf[st][hk], o_acc[db], 0, 0, 0);
          }
      }
    }
    if (t + 1 < ntile) {
      __syncthreads();                 // everyone done reading buf cur^1
      stage_write((t + 1) & 1);        // write-late (T14)
      __syncthreads();
    }
  }

  if (!qvalid) {
    if (VARLEN && qg < S) {       // padded row of a live block
      if (lane < 32) LSE[(long long)bh * S + qg] = 0.f;
      store_zero_row<DH>(Op + (long long)qg * soS, hi);
    }
    return;
  }
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  if (lane < 32) LSE[(long long)bh * S + qg] = m_run + __logf(fmaxf(l_run, 1e-30f));
  store_row<DH, true>(Op + (long long)qg * soS, o_acc, hi, inv);
}

// ---- backward --------------------------------------------------------------

// delta[bh, q] = rowsum(dO o O) — one wave per row, vectorized 16-B loads.
// grid: (ceil(S/4), B*H); one wave per (bh, q) row. DH is a multiple of 8,
// so lanes 0..DH/8-1 each reduce one 16-B chunk.
template <int DH, bool VARLEN>
__global__ __launch_bounds__(THREADS) void flash_delta_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ O,
    float* __restrict__ DELTA, int S, int H,
    long long sdoB, long long sdoS, long long sdoH,
    long long soB, long long soS, long long soH,
    Lens<VARLEN> lens) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int q = blockIdx.x * DELTA_ROWS + wid;
  if (q >= S) return;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  // padded rows are not read; dq and dk/dv never consume their delta
  if (VARLEN && q >= live_len<VARLEN>(lens, b, S)) return;
  const bf16* dop = dO + b * sdoB + h * sdoH + (long long)q * sdoS;
  const bf16* op = O + b * soB + h * soH + (long long)q * soS;
  float acc = 0.f;
  if (lane * 8 < DH) {
    float fd[8], fo[8];
    vload16(dop + lane * 8, fd);
    vload16(op + lane * 8, fo);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(fd[j], fo[j], acc);
  }
  acc = wave_reduce_sum(acc);
  acc = __shfl(acc, 0, 64);
  if (lane == 0) DELTA[(long long)bh * S + q] = acc;
}

// dQ kernel: q-tile-major (same block geometry as forward). Per kv tile:
// recompute P^T from lse, dP^T = mfma(V, dO^T), dS^T, then
// dQ^T += mfma(K^T, dS^T-frags). No atomics: dQ accumulates in registers.
template <int DH, bool CAUSAL, bool VARLEN>
__global__ __launch_bounds__(THREADS) void flash_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dQ, int S, int H, int G, float scale,
    long long sqB, long long sqS, long long sqH,
    long long skB, long long skS, long long skH,
    long long svB, long long svS, long long svH,
    long long sdoB, long long sdoS, long long sdoH,
    long long sdqB, long long sdqS, long long sdqH,
    Lens<VARLEN> lens) {
  constexpr int F = DH / 16;
  constexpr int DB = DH / 32;
  constexpr int NCK = DH / 32;

  // K rows | V rows | K^T — single-buffered (2-phase per tile)
  __shared__ bf16 lds[dq_lds_bytes(DH) / sizeof(bf16)];
  bf16* kb = lds;
  bf16* vb = lds + KVB * DH;
  bf16* ktb = lds + 2 * KVB * DH;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int hi = lane >> 5;
  const int lq = lane & 31;

  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int kvh = h / G;
  const bf16* Qp = Q + b * sqB + h * sqH;
  const bf16* Kp = K + b * skB + kvh * skH;
  const bf16* Vp = V + b * svB + kvh * svH;
  const bf16* dOp = dO + b * sdoB + h * sdoH;
  bf16* dQp = dQ + b * sdqB + h * sdqH;

  const int q0 = blockIdx.x * QB;
  const int qg = q0 + wid * QW + lq;
  const int L = live_len<VARLEN>(lens, b, S);
  if (VARLEN && q0 >= L) {        // dead block: whole block, before any barrier
    if (qg < S) store_zero_row<DH>(dQp + (long long)qg * sdqS, hi);
    return;
  }
  const bool qvalid = qg < L;
  const int qmax_w = min(q0 + wid * QW + QW - 1, L - 1);

  s16x8 qf[F], dof[F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    if (qvalid) {
      qf[f] = *reinterpret_cast<const s16x8*>(
          &Qp[(long long)qg * sqS + f * 16 + hi * 8]);
      dof[f] = *reinterpret_cast<const s16x8*>(
          &dOp[(long long)qg * sdoS + f * 16 + hi * 8]);
    } else {
      qf[f] = s16x8{};
      dof[f] = s16x8{};
    }
  }
  const float lse_q = qvalid ? LSE[(long long)bh * S + qg] : 0.f;
  const float delta_q = qvalid ? DELTA[(long long)bh * S + qg] : 0.f;

  f32x16 dq_acc[DB] = {};

  const int nkv_block = CAUSAL ? min(L, q0 + QB) : L;
  const int ntile = (nkv_block + KVB - 1) / KVB;

  for (int t = 0; t < ntile; ++t) {
    const int k0 = t * KVB;
    // ---- stage K, V (row images) + K^T (transposed) — synchronous
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCK; ++c) {
      const int kv = chunk_row<DH>(c * THREADS + tid);
      const int slot = chunk_slot<DH>(c * THREADS + tid);
      s16x8 kr, vr;
      load_chunk2<DH>(c * THREADS + tid, k0, L, Kp, skS, Vp, svS, kr, vr);
      lds_store128(&kb[koff<DH>(kv, slot * 8)], kr);
      lds_store128(&vb[koff<DH>(kv, slot * 8)], vr);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ktb[voff(slot * 8 + j, kv)] = ((const bf16*)&kr)[j];
    }
    __syncthreads();

    if (CAUSAL && k0 > qmax_w) continue;

    // subtiles processed independently (P comes straight from lse)
    s16x8 dsf[2][2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const s16x8 ak = lds128(&kb[koff<DH>(st * 32 + lq, f * 16 + hi * 8)]);
        const s16x8 av = lds128(&vb[koff<DH>(st * 32 + lq, f * 16 + hi * 8)]);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[f], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, dof[f], dpacc, 0, 0, 0);
      }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_g = k0 + st * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const bool vld = kv_g < L && (!CAUSAL || kv_g <= qg);
        const float p = vld ? __expf(sacc[r] * scale - lse_q) : 0.f;
        ds[r] = p * (dpacc[r] - delta_q) * scale;
      }
#pragma unroll
      for (int hk = 0; hk < 2; ++hk) dsf[st][hk] = pack_frag(ds + hk * 8);
    }
    // dQ^T += K^T x dS^T
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) {
          const s16x8 akt = lds128(
              &ktb[voff(db * 32 + lq, st * 32 + hk * 16 + hi * 8)]);
          dq_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              akt, dsf[st][hk], dq_acc[db], 0, 0, 0);
        }
  }

  if (!qvalid) {
    if (VARLEN && qg < S) store_zero_row<DH>(dQp + (long long)qg * sdqS, hi);
    return;
  }
  store_row<DH>(dQp + (long long)qg * sdqS, dq_acc, hi);
}

// dK/dV kernel: kv-tile-major; each wave owns 32 kv rows of a 128-kv block
// and loops 32-row q tiles in the mirrored orientation (kv lane-local):
// S = mfma(Q, K), dP = mfma(dO, V) — all row-major reads; P/dS fragments
// via the same half-swap; dV^T += mfma(dO^T, P), dK^T += mfma(Q^T, dS).
// Outputs are PER-Q-HEAD (GQA callers group-sum), so no atomics.
template <int DH, bool CAUSAL, bool VARLEN>
__global__ __launch_bounds__(THREADS) void flash_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dK, bf16* __restrict__ dV, int S, int H, int G,
    float scale,
    long long sqB, long long sqS, long long sqH,
    long long skB, long long skS, long long skH,
    long long svB, long long svS, long long svH,
    long long sdoB, long long sdoS, long long sdoH,
    long long sdkB, long long sdkS, long long sdkH,
    long long sdvB, long long sdvS, long long sdvH,
    Lens<VARLEN> lens) {
  constexpr int F = DH / 16;
  constexpr int DB = DH / 32;

  // K rows [128][DH] | V rows [128][DH] | Q [32][DH] | dO [32][DH] |
  // Q^T [DH][32] | dO^T [DH][32]
  __shared__ bf16 lds[dkv_lds_bytes(DH) / sizeof(bf16)];
  bf16* kb = lds;
  bf16* vb = lds + KVBB * DH;
  bf16* qb = lds + 2 * KVBB * DH;
  bf16* dob = qb + 32 * DH;
  bf16* qtb = dob + 32 * DH;
  bf16* dotb = qtb + DH * 32;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int hi = lane >> 5;
  const int lkv = lane & 31;

  const int bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int kvh = h / G;
  const bf16* Qp = Q + b * sqB + h * sqH;
  const bf16* Kp = K + b * skB + kvh * skH;
  const bf16* Vp = V + b * svB + kvh * svH;
  const bf16* dOp = dO + b * sdoB + h * sdoH;
  bf16* dKp = dK + b * sdkB + h * sdkH;
  bf16* dVp = dV + b * sdvB + h * sdvH;

  const int kv0 = blockIdx.x * KVBB;
  const int kv_w = kv0 + wid * 32;            // wave's kv base
  const int kvg = kv_w + lkv;                 // lane's kv row
  const int L = live_len<VARLEN>(lens, b, S);
  if (VARLEN && kv0 >= L) {       // dead block: whole block, before staging
    if (kvg < S) {
      store_zero_row<DH>(dKp + (long long)kvg * sdkS, hi);
      store_zero_row<DH>(dVp + (long long)kvg * sdvS, hi);
    }
    return;
  }
  const bool kvalid = kvg < L;

  // ---- stage block-persistent K/V row images (swizzled)
  // (spelled out like the Q / dO loop below: through load_chunk2 the zeroing
  // of kr and vr swaps places and the main loop is scheduled differently)
  for (int idx = tid; idx < KVBB * DH / 8; idx += THREADS) {
    const int kv = idx / (DH / 8);
    const int slot = idx % (DH / 8);
    const int g = kv0 + kv;
    s16x8 kr = s16x8{}, vr = s16x8{};
    if (g < L) {
      kr = *reinterpret_cast<const s16x8*>(&Kp[(long long)g * skS + slot * 8]);
      vr = *reinterpret_cast<const s16x8*>(&Vp[(long long)g * svS + slot * 8]);
    }
    lds_store128(&kb[koff<DH>(kv, slot * 8)], kr);
    lds_store128(&vb[koff<DH>(kv, slot * 8)], vr);
  }

  f32x16 dv_acc[DB] = {}, dk_acc[DB] = {};

  const int qt0 = CAUSAL ? (kv0 / 32) : 0;    // first q tile that can see kv0
  const int nqt = (L + 31) / 32;

  for (int qt = qt0; qt < nqt; ++qt) {
    const int q0t = qt * 32;
    // ---- stage Q/dO row images + transposes (32 rows). Spelled out: with
    // chunk_row / chunk_slot, load_chunk2 or qtoff in this loop the compiler
    // keeps 8 transposed-write addresses live where this text keeps 4 (4 more
    // VGPRs at dh 32 and 64, other instruction counts)
    __syncthreads();
    {
      const int nchunk = 32 * DH / 8;
      for (int idx = tid; idx < nchunk; idx += THREADS) {
        const int qr = idx / (DH / 8);
        const int slot = idx % (DH / 8);
        const int g = q0t + qr;
        s16x8 qr16 = s16x8{}, dor16 = s16x8{};
        if (g < L) {
          qr16 = *reinterpret_cast<const s16x8*>(
              &Qp[(long long)g * sqS + slot * 8]);
          dor16 = *reinterpret_cast<const s16x8*>(
              &dOp[(long long)g * sdoS + slot * 8]);
        }
        lds_store128(&qb[koff<DH>(qr, slot * 8)], qr16);
        lds_store128(&dob[koff<DH>(qr, slot * 8)], dor16);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d = slot * 8 + j;
          qtb[d * 32 + ((((qr >> 3) ^ d) & 3) << 3) + (qr & 7)] =
              ((const bf16*)&qr16)[j];
          dotb[d * 32 + ((((qr >> 3) ^ d) & 3) << 3) + (qr & 7)] =
              ((const bf16*)&dor16)[j];
        }
      }
    }
    __syncthreads();

    if (CAUSAL && q0t + 31 < kv_w) continue;  // wave sees nothing here

    // ---- S = Q x K^T and dP = dO x V^T (kv lane-local)
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const s16x8 aq = lds128(&qb[koff<DH>(lkv, f * 16 + hi * 8)]);
      const s16x8 ado = lds128(&dob[koff<DH>(lkv, f * 16 + hi * 8)]);
      const s16x8 bk = lds128(&kb[koff<DH>(wid * 32 + lkv, f * 16 + hi * 8)]);
      const s16x8 bv = lds128(&vb[koff<DH>(wid * 32 + lkv, f * 16 + hi * 8)]);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq, bk, sacc, 0, 0, 0);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ado, bv, dpacc, 0, 0, 0);
    }
    float pv[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q_g = q0t + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const bool vld = q_g < L && kvalid && (!CAUSAL || kvg <= q_g);
      float lse_r = 0.f, del_r = 0.f;
      if (vld) {
        lse_r = LSE[(long long)bh * S + q_g];
        del_r = DELTA[(long long)bh * S + q_g];
      }
      const float p = vld ? __expf(sacc[r] * scale - lse_r) : 0.f;
      pv[r] = p;
      ds[r] = p * (dpacc[r] - del_r) * scale;
    }
    // fragments over q (half-swap, q consecutive)
    s16x8 pfr[2], dsfr[2];
#pragma unroll
    for (int hk = 0; hk < 2; ++hk) {
      const int o8 = hk * 8;
      pfr[hk] = pack_frag(pv + o8);
      dsfr[hk] = pack_frag(ds + o8);
    }
    // dV^T += dO^T x P ; dK^T += Q^T x dS
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int hk = 0; hk < 2; ++hk) {
        const int off = qtoff(db * 32 + lkv, hk * 16 + hi * 8);
        const s16x8 adot = lds128(&dotb[off]);
        const s16x8 aqt = lds128(&qtb[off]);
        dv_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            adot, pfr[hk], dv_acc[db], 0, 0, 0);
        dk_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            aqt, dsfr[hk], dk_acc[db], 0, 0, 0);
      }
  }

  if (!kvalid) {
    if (VARLEN && kvg < S) {      // padded row of a live block
      store_zero_row<DH>(dKp + (long long)kvg * sdkS, hi);
      store_zero_row<DH>(dVp + (long long)kvg * sdvS, hi);
    }
    return;
  }
  bf16* dkrow = dKp + (long long)kvg * sdkS;
  bf16* dvrow = dVp + (long long)kvg * sdvS;
  // store_row twice, run by run, spelled out: two calls in sequence cost
  // VARLEN 20+ instructions, and any helper here reorders the main loop
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int d0 = db * 32 + qd * 8 + hi * 4;
      const unsigned int k0w =
          pk_bf16(dk_acc[db][qd * 4 + 0], dk_acc[db][qd * 4 + 1]);
      const unsigned int k1w =
          pk_bf16(dk_acc[db][qd * 4 + 2], dk_acc[db][qd * 4 + 3]);
      const unsigned int v0w =
          pk_bf16(dv_acc[db][qd * 4 + 0], dv_acc[db][qd * 4 + 1]);
      const unsigned int v1w =
          pk_bf16(dv_acc[db][qd * 4 + 2], dv_acc[db][qd * 4 + 3]);
      *reinterpret_cast<u32x2*>(&dkrow[d0]) = u32x2{k0w, k1w};
      *reinterpret_cast<u32x2*>(&dvrow[d0]) = u32x2{v0w, v1w};
    }
}

// Host dispatch: f(dh, causal, varlen) gets the three as integral constants,
// varlen being "a has seq_lens"; nothing runs for a route that refuses.
template <typename F>
void dispatch(const FlashRoute& rt, int DH, bool causal, const FlashArgs& a,
              F&& f) {
  if (!rt.eligible) throw std::runtime_error(rt.refusal);
  dispatch2(causal, a.seq_lens != nullptr, [&](auto cz, auto vl) {
    if (DH == 32) f(std::integral_constant<int, 32>{}, cz, vl);
    else if (DH == 64) f(std::integral_constant<int, 64>{}, cz, vl);
    else f(std::integral_constant<int, 128>{}, cz, vl);
  });
}

// seq_lens for VARLEN, the empty struct for the dense instantiations
template <bool VL> Lens<VL> lens_arg(const int* seq_lens) {
  if constexpr (VL) return seq_lens; else return NoLens{};
}

}  // namespace fa

// Each launcher launches the grid the route names, with the strides of the
// problem's views. a.seq_lens == nullptr launches the dense instantiations
// (empty-struct last argument), else the VARLEN ones on the same grid.

void launch_flash_fwd(const FlashRoute& rt, const FlashProblem& p,
                      const FlashArgs& a, float scale, hipStream_t s) {
  const AttnView *q = &p.view[kQ], *k = &p.view[kK], *v = &p.view[kV],
                 *o = &p.view[kO];
  fa::dispatch(rt, p.DH, p.causal, a, [&](auto dh, auto cz, auto vl) {
    constexpr int DH = decltype(dh)::value;
    constexpr bool CZ = decltype(cz)::value, VL = decltype(vl)::value;
    hipLaunchKernelGGL((fa::flash_fwd_kernel<DH, CZ, VL>),
                       dim3(rt.grid_fwd[0], rt.grid_fwd[1]), dim3(fa::THREADS),
                       0, s, (const bf16*)a.q, (const bf16*)a.k,
                       (const bf16*)a.v, (bf16*)a.o, a.lse, p.S, p.H, rt.G,
                       scale, q->sB, q->sS, q->sH, k->sB, k->sS, k->sH, v->sB,
                       v->sS, v->sH, o->sB, o->sS, o->sH,
                       fa::lens_arg<VL>(a.seq_lens));
  });
}

void launch_flash_delta(const FlashRoute& rt, const FlashProblem& p,
                        const FlashArgs& a, hipStream_t s) {
  const AttnView *dO = &p.view[kDout], *o = &p.view[kO];
  fa::dispatch(rt, p.DH, false, a, [&](auto dh, auto, auto vl) {
    constexpr int DH = decltype(dh)::value;
    constexpr bool VL = decltype(vl)::value;
    hipLaunchKernelGGL((fa::flash_delta_kernel<DH, VL>),
                       dim3(rt.grid_delta[0], rt.grid_delta[1]),
                       dim3(fa::THREADS), 0, s, (const bf16*)a.dout,
                       (const bf16*)a.o, a.delta, p.S, p.H, dO->sB, dO->sS,
                       dO->sH, o->sB, o->sS, o->sH,
                       fa::lens_arg<VL>(a.seq_lens));
  });
}

void launch_flash_bwd_dq(const FlashRoute& rt, const FlashProblem& p,
                         const FlashArgs& a, float scale, hipStream_t s) {
  const AttnView *q = &p.view[kQ], *k = &p.view[kK], *v = &p.view[kV],
                 *dO = &p.view[kDout], *dq = &p.view[kDq];
  fa::dispatch(rt, p.DH, p.causal, a, [&](auto dh, auto cz, auto vl) {
    constexpr int DH = decltype(dh)::value;
    constexpr bool CZ = decltype(cz)::value, VL = decltype(vl)::value;
    hipLaunchKernelGGL((fa::flash_bwd_dq_kernel<DH, CZ, VL>),
                       dim3(rt.grid_dq[0], rt.grid_dq[1]), dim3(fa::THREADS),
                       0, s, (const bf16*)a.q, (const bf16*)a.k,
                       (const bf16*)a.v, (const bf16*)a.dout, a.lse, a.delta,
                       (bf16*)a.dq, p.S, p.H, rt.G, scale, q->sB, q->sS, q->sH,
                       k->sB, k->sS, k->sH, v->sB, v->sS, v->sH, dO->sB,
                       dO->sS, dO->sH, dq->sB, dq->sS, dq->sH,
                       fa::lens_arg<VL>(a.seq_lens));
  });
}

void launch_flash_bwd_dkv(const FlashRoute& rt, const FlashProblem& p,
                          const FlashArgs& a, float scale, hipStream_t s) {
  const AttnView *q = &p.view[kQ], *k = &p.view[kK], *v = &p.view[kV],
                 *dO = &p.view[kDout], *dk = &p.view[kDk], *dv = &p.view[kDv];
  fa::dispatch(rt, p.DH, p.causal, a, [&](auto dh, auto cz, auto vl) {
    constexpr int DH = decltype(dh)::value;
    constexpr bool CZ = decltype(cz)::value, VL = decltype(vl)::value;
    hipLaunchKernelGGL((fa::flash_bwd_dkv_kernel<DH, CZ, VL>),
                       dim3(rt.grid_dkv[0], rt.grid_dkv[1]), dim3(fa::THREADS),
                       0, s, (const bf16*)a.q, (const bf16*)a.k,
                       (const bf16*)a.v, (const bf16*)a.dout, a.lse, a.delta,
                       (bf16*)a.dk, (bf16*)a.dv, p.S, p.H, rt.G, scale, q->sB,
                       q->sS, q->sH, k->sB, k->sS, k->sH, v->sB, v->sS, v->sH,
                       dO->sB, dO->sS, dO->sH, dk->sB, dk->sS, dk->sH, dv->sB,
                       dv->sS, dv->sH, fa::lens_arg<VL>(a.seq_lens));
  });
}

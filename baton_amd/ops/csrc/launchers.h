// Host-side launcher declarations: the boundary between the torch binding
// layer (bindings.cpp) and the HIP kernel TUs. Raw pointers + hipStream_t
// only — keeps torch headers out of kernel compiles.
#pragma once
#include <hip/hip_runtime.h>

#include "attn_route.h"
#include "conv_route.h"
#include "gemm_plan.h"
#include "gemm_strides.h"
#include "norm_route.h"

// optim.hip
void launch_sgd(bool is_bf16, void* p, void* g, float* m, long long n,
                float lr, float momentum, float wd, int zero_after,
                hipStream_t s);
void launch_adam(bool is_bf16, void* p, void* g, float* m, float* v,
                 long long n, float lr, float b1, float b2, float eps, float wd,
                 float inv_bc1, float inv_sqrt_bc2, int zero_after,
                 hipStream_t s);
// Blocks of the step and sumsq kernels for n elements: what grad_sumsq writes.
int optim_grid(long long n);
// The EXT steps: clip_state (may be null) as clip_finalize wrote it.
void launch_sgd_ext(bool is_bf16, void* p, void* g, float* m, long long n,
                    float lr, float momentum, float wd, int zero_after,
                    const float* clip_state, int decoupled, hipStream_t s);
void launch_adam_ext(bool is_bf16, void* p, void* g, float* m, float* v,
                     long long n, float lr, float b1, float b2, float eps,
                     float wd, float inv_bc1, float inv_sqrt_bc2,
                     int zero_after, const float* clip_state, int decoupled,
                     hipStream_t s);
// One fp32 partial per block at partials[0 .. grid); returns the grid.
int launch_grad_sumsq(bool is_bf16, const void* g, long long n,
                      float* partials, hipStream_t s);
void launch_clip_finalize(const float* partials, int count, double max_norm,
                          float* clip_state, hipStream_t s);

// fedmath.hip
void launch_scale_cast(bool src_bf16, float* dst, const void* src, long long n,
                       float alpha, hipStream_t s);
void launch_cast_copy(bool dst_bf16, void* dst, const float* src, long long n,
                      hipStream_t s);
void launch_axpby(float* y, const float* x, long long n, float a, float b,
                  hipStream_t s);

// fedopt.hip — the federated server step. All of x, m, v, D, dst, partials,
// clip_state, w_sum / w_out and round_state are fp32; theta is fp32 or bf16.
// One fp32 partial per block of sum (float(theta) - x)^2 at
// partials[0 .. grid); returns the grid (optim_grid(n)).
int launch_delta_sumsq(bool is_bf16, const void* theta, const float* x,
                       long long n, float* partials, hipStream_t s);
// dst = (alpha * clip_state[1]) * (float(theta) - x), or +0.0 without a read
// of theta when clip_state[2] == 0; w_out (may be null) = alpha or 0.
void launch_delta_scale_cast(bool is_bf16, float* dst, const void* theta,
                             const float* x, long long n, float alpha,
                             const float* clip_state, float* w_out,
                             hipStream_t s);
// round_state[4] = [W, 1 / W or 0, applied 1 / 0, skipped rounds] from w_sum[0]
void launch_fedopt_finalize(const float* w_sum, float* round_state,
                            hipStream_t s);
// mode: 0 mean (m, v null), 1 fedavgm (v null), 2 fedadagrad, 3 fedadam,
// 4 fedyogi. Updates x, m, v in place; nothing when round_state[2] == 0.
void launch_server_step(int mode, const float* D, float* x, float* m, float* v,
                        long long n, float lr, float b1, float b2, float tau,
                        const float* round_state, hipStream_t s);
// The same step with DP noise: Delta = fl(D + fl(sigma * zeta)), zeta the
// Philox4x32-10 unit normal of (seed, round, stream, elem_offset + e); inv_W
// is not read. elem_offset is a multiple of 4 (fed/server_opt.py).
void launch_server_step_noise(int mode, const float* D, float* x, float* m,
                              float* v, long long n, float lr, float b1,
                              float b2, float tau, const float* round_state,
                              unsigned long long seed, unsigned round,
                              unsigned stream, long long elem_offset,
                              float sigma, hipStream_t s);
// out[e] = fl(sigma * zeta) alone, on the step's index walk.
void launch_dp_noise(float* out, long long n, unsigned long long seed,
                     unsigned round, unsigned stream, long long elem_offset,
                     float sigma, hipStream_t s);

// fedrobust.hip — coordinate-wise median and trimmed mean in front of the
// server step. flags (fp32, live iff != 0), round_state[4] and agg_state[2]
// are fp32, b_table is int32 with K + 1 entries.
// round_state = [kept, 1 / kept or 0, applied 1 / 0, skipped rounds] and
// agg_state = [k live rows, b = b_table[k]] from flags[0 .. K).
void launch_robust_finalize(const float* flags, const int* b_table, int K,
                            float* round_state, float* agg_state,
                            hipStream_t s);
// D[e] = the ascending sequential sum of the sorted live U[0 .. K)[e] from
// rank b to rank k - b - 1; K in 1 .. 16, rows `stride` elements apart (a
// multiple of 4). Nothing is written when round_state[2] == 0.
void launch_robust_select(int K, float* D, const float* U, long long stride,
                          long long n, const float* flags,
                          const float* agg_state, const float* round_state,
                          hipStream_t s);

// loss.hip
void launch_mse_fwd(bool is_bf16, const void* x, const void* y, float* out,
                    long long n, hipStream_t s);
void launch_scale_scalar(float* out, float scale, hipStream_t s);
void launch_mse_bwd(bool is_bf16, const void* x, const void* y,
                    const float* dout, void* dx, long long n, hipStream_t s);
void launch_ce_fwd(bool is_bf16, const void* logits, const long long* target,
                   float* lse, float* loss_sum, int B, int C, hipStream_t s);
void launch_ce_bwd(bool is_bf16, const void* logits, const long long* target,
                   const float* lse, const float* dout, void* dx, int B, int C,
                   hipStream_t s);
// ignored labels: rows with target outside [0, C) or == ignore_index are
// skipped; loss = mean over the live rows (0 when none), n_valid = their count,
// both zeroed by the caller
void launch_ce_masked_fwd(bool is_bf16, const void* logits,
                          const long long* target, float* lse, float* loss,
                          int* n_valid, long long ignore_index, int B, int C,
                          hipStream_t s);
void launch_ce_masked_bwd(bool is_bf16, const void* logits,
                          const long long* target, const float* lse,
                          const int* n_valid, const float* dout, void* dx,
                          long long ignore_index, int B, int C, hipStream_t s);

// norm.hip — LayerNorm (center) / RMSNorm rows and BatchNorm: each launches
// exactly the grid, kernel form and LDS size the route names (norm_route.h
// decides). res / plus / dres select the fused forms when not nullptr; b,
// mean and db are LayerNorm's alone.
void launch_norm_fwd(const NormRowRoute& rt, bool is_bf16, bool center,
                     const void* x, const void* res, const void* w,
                     const void* b, void* y, void* zout, float* mean,
                     float* rstd, long long R, int C, float eps, hipStream_t s);
void launch_norm_bwd(const NormRowRoute& rt, bool is_bf16, bool center,
                     const void* x, const void* dy, const void* w,
                     const float* mean, const float* rstd, const void* plus,
                     void* dx, float* dw, float* db, long long R, int C,
                     hipStream_t s);
void launch_bn_stats(const BnRoute& rt, bool is_bf16, const void* x, float* sum,
                     float* sumsq, long long M, int C, hipStream_t s);
void launch_bn_finalize(const float* sum, const float* sumsq, float* mean,
                        float* rstd, float* running_mean, float* running_var,
                        long long M, int C, float eps, float momentum,
                        hipStream_t s);
void launch_bn_norm(const BnRoute& rt, bool is_bf16, bool relu, const void* x,
                    const void* res, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, void* y, long long M,
                    int C, hipStream_t s);
void launch_bn_bwd_stats(const BnRoute& rt, bool is_bf16, bool relu,
                         const void* x, const void* dy, const void* y_post,
                         const float* mean, const float* rstd, float* sum_dy,
                         float* sum_dyx, long long M, int C, hipStream_t s);
void launch_bn_bwd_dx(const BnRoute& rt, bool is_bf16, bool relu, const void* x,
                      const void* dy, const void* y_post, const float* mean,
                      const float* rstd, const float* gamma,
                      const float* sum_dy, const float* sum_dyx, void* dx,
                      void* dres, long long M, int C, hipStream_t s);

// elementwise.hip
void launch_relu_fwd(bool is_bf16, const void* x, void* y, long long n,
                     hipStream_t s);
void launch_relu_bwd(bool is_bf16, const void* dy, const void* y, void* dx,
                     long long n, hipStream_t s);
void launch_add_relu_fwd(bool is_bf16, const void* a, const void* b, void* y,
                         long long n, hipStream_t s);
void launch_add_scaled_fwd(bool is_bf16, const void* a, const void* b, void* z,
                           float alpha, long long n, hipStream_t s);
void launch_scale_fwd(bool is_bf16, const void* x, void* z, float alpha,
                      long long n, hipStream_t s);
void launch_gelu_fwd(bool is_bf16, const void* x, void* y, long long n,
                     hipStream_t s);
void launch_gelu_bwd(bool is_bf16, const void* dy, const void* x, void* dx,
                     long long n, hipStream_t s);

// Conv launchers (conv.hip, conv8.hip, conv_halo.hip, conv_wgrad_px.hip):
// each launches exactly the kernel, tile, grid and pixel split the ConvRoute
// names (conv_route.h decides) and returns false, launching nothing, when
// the route is not its kind or its kernel cannot run the problem.

// conv.hip — NHWC implicit GEMM. Generic fwd; Generic / DgradPhase dgrad (w
// is the [Cin,KH,KW,Cout] transposed copy); WgradGeneric (dy is the
// TRANSPOSED [Cout][P] copy, dw the zeroed fp32 buffer).
bool launch_conv_fwd(const ConvRoute& rt, const ConvProblem& p, const void* x,
                     const void* w, void* y, hipStream_t s);
bool launch_conv_dgrad(const ConvRoute& rt, const ConvProblem& p,
                       const void* dy, const void* w_t, void* dx,
                       hipStream_t s);
bool launch_conv_wgrad(const ConvRoute& rt, const ConvProblem& p,
                       const void* dy_t, const void* x, void* dw,
                       hipStream_t s);

// GEMM launchers (gemm.hip, gemm8.hip): each launches exactly the kernel,
// tile, grid and K split the GemmPlan names (gemm_plan.h decides) and
// returns false, launching nothing, when the plan does not fit the problem.
// Layout comes from the plan: 0 = NT (fwd), 1 = NN (dgrad), 2 = TN (wgrad).

// gemm.hip — 2-phase kernel, dense; batched via grid.z = nbatch with
// per-batch element strides (attention)
bool launch_gemm_2ph(const GemmPlan& pl, const GemmProblem& p, const void* A,
                     const void* B, void* C, const float* bias,
                     long long strideA, long long strideB, long long strideC,
                     hipStream_t s, int b_group = 1,
                     GemmStrides gs = GemmStrides{0, 0, 0, 1, 0, 0, 0});

// gemm.hip — 2-phase split-K: fp32 atomic accumulation over K slices into
// a zeroed C
bool launch_gemm_2ph_splitk(const GemmPlan& pl, bool in_bf16, const void* A,
                            const void* B, float* C, int M, int N, int K,
                            hipStream_t s);

// gemm8.hip — deep-pipelined 256x256 8-wave NT kernel (bf16 full tiles),
// fused fp32 bias
bool launch_gemm_nt_g9(const GemmPlan& pl, const void* A, const void* B,
                       void* C, const float* bias, int M, int N, int K,
                       float alpha, hipStream_t s);

// gemm8.hip — 8-wave split-K: per-slice fp32 slabs + reduce (no atomics)
bool launch_gemm_nt_slab(const GemmPlan& pl, const void* A, const void* B,
                         float* slabs, void* out, bool out_bf16, int M, int N,
                         int K, hipStream_t s);

// attention.hip — row softmax with scale + optional causal mask and optional
// per-sequence key lengths: kv_len is nullptr, or device int32 lengths where
// rows_per_len consecutive rows share one entry and r % q_period is a row's
// query position. Kernel and grid are softmax_route's (attn_route.h).
void launch_softmax_fwd(bool is_bf16, const void* x, void* y, long long R,
                        int C, float scale, int causal_seq, const int* kv_len,
                        long long rows_per_len, int q_period, hipStream_t s);
void launch_softmax_bwd(bool is_bf16, const void* y, const void* dy, void* dx,
                        long long R, int C, float scale, hipStream_t s);

// llama_ops.hip — RoPE / SwiGLU
void launch_rope(bool is_bf16, bool inverse, const void* x, void* y,
                 const float* cos_t, const float* sin_t, long long total_pairs,
                 int S, int H, int D, hipStream_t s);
void launch_silu_mul_fwd(bool is_bf16, const void* a, const void* b, void* y,
                         long long n, hipStream_t s);
void launch_silu_mul_bwd(bool is_bf16, const void* dy, const void* a,
                         const void* b, void* da, void* db, long long n,
                         hipStream_t s);

// fedmath.hip — LDS-tiled matrix transpose [R,C] -> [C,R]
void launch_transpose(bool is_bf16, const void* in, void* out, int R, int C,
                      hipStream_t s);

// fedmath.hip — column sum (bias gradients): out[c] = sum_r x[r,c], fp32
void launch_colsum(bool is_bf16, const void* x, float* out, long long R, int C,
                   hipStream_t s);

// flash.hip — fused flash attention. Each launcher launches the grid the
// route (flash_route of the problem, attn_route.h) names, with the strides of
// the problem's views, and throws on a route that is not eligible. seq_lens:
// nullptr (the dense kernels), or B device int32 lengths of right-padded
// sequences (the length-aware instantiations).
struct FlashArgs {
  const void *q, *k, *v, *dout;   // dout, delta, dq, dk, dv: backward only
  void *o, *dq, *dk, *dv;
  float *lse, *delta;
  const int* seq_lens;
};
void launch_flash_fwd(const FlashRoute& rt, const FlashProblem& p,
                      const FlashArgs& a, float scale, hipStream_t s);
void launch_flash_delta(const FlashRoute& rt, const FlashProblem& p,
                        const FlashArgs& a, hipStream_t s);
void launch_flash_bwd_dq(const FlashRoute& rt, const FlashProblem& p,
                         const FlashArgs& a, float scale, hipStream_t s);
void launch_flash_bwd_dkv(const FlashRoute& rt, const FlashProblem& p,
                          const FlashArgs& a, float scale, hipStream_t s);

// conv8.hip — deep-pipelined 256x256 8-wave conv fwd / stride-1 dgrad
// (bf16; p.op picks). b is w for fwd, the transposed w_t for dgrad.
bool launch_conv_8ph(const ConvRoute& rt, const ConvProblem& p, const void* a,
                     const void* b, void* out, hipStream_t s);

// conv_halo.hip — shared-halo 3x3 stride-1 conv fwd / dgrad (p.op picks) for
// small-channel layers whose 128-px tiles stay within one image. wf is the
// fragment-ordered image of w (fwd) / w_t (dgrad).
bool launch_conv_halo(const ConvRoute& rt, const ConvProblem& p, const void* a,
                      const void* wf, void* out, hipStream_t s);

// conv_wgrad_px.hip — pixel-major tap-shared 3x3 stride-1 wgrad: dy in its
// natural [P][Cout] layout, dw the zeroed fp32 buffer
bool launch_conv_wgrad_px(const ConvRoute& rt, const ConvProblem& p,
                          const void* dy, const void* x, void* dw,
                          hipStream_t s);

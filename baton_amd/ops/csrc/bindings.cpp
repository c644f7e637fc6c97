// torch bindings for the baton_amd gfx950 kernels.
//
// Validate tensors (contiguous, dtype, device), allocate outputs and
// workspaces, pull raw pointers and the current HIP stream, call the
// launchers (launchers.h). Every FLOP is in the .hip kernels; the policy
// executed here is the GEMM plan (gemm_plan.h) and the conv route
// (conv_route.h): gemm() and conv_fwd() / conv_dgrad() / conv_wgrad()
// allocate what the plan asks for and launch what it names.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <limits>

#include "launchers.h"
#include "wgrad_px_map.h"
#include "dgrad_phase_map.h"

namespace {

bool is_bf16(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16; }

void check_compute(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16,
              name, " must be fp32 or bf16");
}

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

// Refuse what no kernel is instantiated for, before anything is allocated
// or launched.
void check_supported(const GemmProblem& p, const GemmPlan& pl) {
  const char* why = gemm_unsupported(p, pl);
  TORCH_CHECK(why == nullptr, "gemm: unsupported combination: ", why ? why : "",
              " (layout ", p.layout, ", ", kGemmKindName[(int)pl.kind], " plan)");
}

// Execute a plan_dense() plan: the 2-phase kernel, or G9 plus (ragged M)
// the remainder rows under their own plan.
void run_dense(const GemmProblem& p, const GemmPlan& pl, const void* A,
               const void* B, void* C, const float* bias, long long strideA = 0,
               long long strideB = 0, long long strideC = 0, int b_group = 1,
               GemmStrides gs = GemmStrides{0, 0, 0, 1, 0, 0, 0}) {
  if (pl.kind == GemmKind::G9) {
    TORCH_CHECK(launch_gemm_nt_g9(pl, A, B, C, bias, pl.m_main, p.N, p.K,
                                  (float)p.alpha, stream()),
                "gemm: G9 plan does not fit ", pl.m_main, "x", p.N, "x", p.K);
    if (pl.m_main == p.M) return;
    const GemmProblem r = gemm_remainder(p, pl);
    run_dense(r, plan_dense(r),
              (const at::BFloat16*)A + (long long)pl.m_main * p.K, B,
              (at::BFloat16*)C + (long long)pl.m_main * p.N, bias);
    return;
  }
  TORCH_CHECK(launch_gemm_2ph(pl, p, A, B, C, bias, strideA, strideB, strideC,
                              stream(), b_group, gs),
              "gemm: 2-phase plan does not fit ", p.M, "x", p.N, "x", p.K);
}

// The split-K executors gemm() and the 1x1 conv wgrad share. A, B are NT
// operands; out is [M, N], for the atomic route fp32 and zeroed.
void run_slab(const GemmPlan& pl, const at::Tensor& A, const at::Tensor& B,
              at::Tensor& out, int M, int N, int K) {
  auto slabs = at::empty({(long long)pl.splits * M * N},
                         A.options().dtype(at::kFloat));
  TORCH_CHECK(launch_gemm_nt_slab(pl, A.data_ptr(), B.data_ptr(),
                                  slabs.data_ptr<float>(), out.data_ptr(),
                                  out.scalar_type() != at::kFloat, M, N, K,
                                  stream()),
              "gemm: slab plan does not fit ", M, "x", N, "x", K);
}

void run_splitk(const GemmPlan& pl, const at::Tensor& A, const at::Tensor& B,
                at::Tensor& out, int M, int N, int K) {
  TORCH_CHECK(launch_gemm_2ph_splitk(pl, is_bf16(A), A.data_ptr(), B.data_ptr(),
                                     out.data_ptr<float>(), M, N, K, stream()),
              "gemm: split-K plan does not fit ", M, "x", N, "x", K);
}

// A conv launcher that refuses its route is a bug in conv_route.h, never a
// reason to run another kernel.
void check_launched(bool ok, const ConvProblem& p, const ConvRoute& rt) {
  TORCH_CHECK(ok, "conv ", kConvOpName[(int)p.op], ": ",
              kConvKindName[(int)rt.kind], " route does not fit N=", p.N,
              " H=", p.H, " W=", p.W, " Cin=", p.Cin, " Cout=", p.Cout, " K=",
              p.KH, "x", p.KW, " stride=", p.stride, " pad=", p.pad);
}

// ---- normalization argument checks ----------------------------------------
// The norm kernels take raw pointers and trust (R, C): everything they read
// or write is sized here, before anything is allocated or launched.

struct NormShape {
  long long R;   // rows (LayerNorm / RMSNorm) or samples per channel (BN)
  int C;
};

// x: fp32 / bf16, contiguous, on the GPU, viewed as [R, C] with both > 0.
// rows_fit_int: the LayerNorm kernels index rows with int.
NormShape norm_shape(const at::Tensor& x, const char* op, bool rows_fit_int) {
  check_compute(x, "x");
  TORCH_CHECK(x.dim() >= 1, op, ": x must have at least one dimension");
  const long long C = x.size(-1);
  TORCH_CHECK(C > 0, op, ": x has C == 0 channels");
  TORCH_CHECK(x.numel() > 0, op, ": x has no rows");
  TORCH_CHECK(C <= INT_MAX, op, ": x has C = ", C, ", past the kernels' int");
  const long long R = x.numel() / C;
  TORCH_CHECK(!rows_fit_int || R <= INT_MAX, op, ": x has ", R,
              " rows, past the kernels' int");
  return {R, (int)C};
}

// A second tensor that must match the first one (xs names it as a possessive,
// "x's"): its device, dtype and contiguity, and its sizes (flat: its element
// count, for the streaming ops).
void check_like(const at::Tensor& t, const char* name, const at::Tensor& x,
                const char* xs, const char* op, bool flat = false) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), op, ": ", name,
              " must be on ", xs, " device");
  TORCH_CHECK(t.scalar_type() == x.scalar_type(), op, ": ", name,
              " must have ", xs, " dtype");
  if (flat) {
    TORCH_CHECK(t.numel() == x.numel(), op, ": ", name, " must have ", xs, " ",
                x.numel(), " elements, got ", t.numel());
  } else {
    TORCH_CHECK(t.sizes() == x.sizes(), op, ": ", name, " must have ", xs,
                " sizes ", x.sizes(), ", got ", t.sizes());
  }
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// A contiguous buffer of exactly n elements of dtype dt on the device of x.
void check_vec(const at::Tensor& t, const char* name, const at::Tensor& x,
               const char* xs, at::ScalarType dt, long long n,
               const char* op) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), op, ": ", name,
              " must be on ", xs, " device");
  TORCH_CHECK(t.scalar_type() == dt, op, ": ", name, " must be ",
              dt == at::kFloat  ? "fp32"
              : dt == at::kLong ? "int64"
                                : "of x's dtype");
  TORCH_CHECK(t.numel() == n, op, ": ", name, " must have ", n,
              " elements, got ", t.numel());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// dy / res / plus / y_post: x's sizes, dtype and device, contiguous.
void norm_check_like_x(const at::Tensor& t, const char* name,
                       const at::Tensor& x, const char* op) {
  check_like(t, name, x, "x's", op);
}

// w / b (x's dtype), mean / rstd / gamma / beta / running statistics (fp32).
void norm_check_vec(const at::Tensor& t, const char* name, const at::Tensor& x,
                    at::ScalarType dt, long long n, const char* op) {
  check_vec(t, name, x, "x's", dt, n, op);
}

// The first tensor of a streaming op: fp32 / bf16, contiguous, on the GPU.
void check_first(const at::Tensor& t, const char* name, const char* op) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16,
              op, ": ", name, " must be fp32 or bf16");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

bool norm_absent(const at::Tensor& t) { return !t.defined() || t.numel() == 0; }

}  // namespace

// ---- optim -----------------------------------------------------------------

void sgd_step(at::Tensor p, at::Tensor g, at::Tensor m, double lr,
              double momentum, double weight_decay, bool zero_grad) {
  check_compute(p, "p");
  check_compute(g, "g");
  TORCH_CHECK(p.scalar_type() == g.scalar_type(), "p/g dtype mismatch");
  TORCH_CHECK(p.numel() == g.numel(), "p/g numel mismatch");
  float* mptr = nullptr;
  if (m.defined() && m.numel() > 0) {
    TORCH_CHECK(m.scalar_type() == at::kFloat && m.is_contiguous());
    TORCH_CHECK(m.numel() == p.numel());
    mptr = m.data_ptr<float>();
  }
  launch_sgd(is_bf16(p), p.data_ptr(), g.data_ptr(), mptr, p.numel(), (float)lr,
             (float)momentum, (float)weight_decay, zero_grad ? 1 : 0,
             stream());
}

void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
               double lr, double beta1, double beta2, double eps,
               double weight_decay, double bc1, double bc2, bool zero_grad) {
  check_compute(p, "p");
  check_compute(g, "g");
  TORCH_CHECK(m.scalar_type() == at::kFloat && v.scalar_type() == at::kFloat);
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() &&
              p.numel() == v.numel());
  launch_adam(is_bf16(p), p.data_ptr(), g.data_ptr(), m.data_ptr<float>(),
              v.data_ptr<float>(), p.numel(), (float)lr, (float)beta1,
              (float)beta2, (float)eps, (float)weight_decay,
              (float)(1.0 / bc1), (float)(1.0 / std::sqrt(bc2)),
              zero_grad ? 1 : 0, stream());
}

// Clipping, the non-finite skip and decoupled decay (optim.hip). Everything
// these ops refuse is refused here, before any launch, by argument name.

namespace {

// p / g / m / v of the new ops: on the GPU, contiguous, 16-byte aligned.
void optim_check_buf(const at::Tensor& t, const char* name, const char* op) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ",
              name, " must be 16-byte aligned");
}

void optim_check_pg(const at::Tensor& p, const at::Tensor& g, const char* op) {
  optim_check_buf(p, "p", op);
  optim_check_buf(g, "g", op);
  TORCH_CHECK(p.scalar_type() == at::kFloat || p.scalar_type() == at::kBFloat16,
              op, ": p must be fp32 or bf16");
  TORCH_CHECK(g.scalar_type() == p.scalar_type(), op, ": g must have p's dtype");
  TORCH_CHECK(g.device() == p.device(), op, ": g must be on p's device");
  TORCH_CHECK(g.numel() == p.numel(), op, ": g must have p's ", p.numel(),
              " elements, got ", g.numel());
}

// fp32 moment of p's size on p's device
void optim_check_moment(const at::Tensor& t, const char* name,
                        const at::Tensor& p, const char* op) {
  optim_check_buf(t, name, op);
  TORCH_CHECK(t.device() == p.device(), op, ": ", name,
              " must be on p's device");
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.numel() == p.numel(), op, ": ", name, " must have p's ",
              p.numel(), " elements, got ", t.numel());
}

// partials / clip_state: contiguous fp32 on dev
void optim_check_f32(const at::Tensor& t, const char* name, c10::Device dev,
                     const char* op) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda() && t.device() == dev, op, ": ", name,
              " must be on the gradients' device");
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

const float* optim_clip_state(const c10::optional<at::Tensor>& cs,
                              const at::Tensor& p, const char* op) {
  if (!cs.has_value() || !cs->defined()) return nullptr;
  optim_check_f32(*cs, "clip_state", p.device(), op);
  TORCH_CHECK(cs->numel() == 4, op, ": clip_state must have 4 elements, got ",
              cs->numel());
  return cs->data_ptr<float>();
}

}  // namespace

long long optim_grid_py(long long n) {
  TORCH_CHECK(n >= 0, "optim_grid: n must be >= 0");
  return optim_grid(n);
}

long long grad_sumsq(at::Tensor g, at::Tensor partials, long long offset) {
  const char* op = "grad_sumsq";
  optim_check_buf(g, "g", op);
  TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16,
              op, ": g must be fp32 or bf16");
  optim_check_f32(partials, "partials", g.device(), op);
  const long long nblocks = optim_grid(g.numel());
  TORCH_CHECK(offset >= 0 && offset + nblocks <= partials.numel(), op,
              ": offset ", offset, " + ", nblocks, " blocks is beyond partials (",
              partials.numel(), " elements)");
  launch_grad_sumsq(is_bf16(g), g.data_ptr(), g.numel(),
                    partials.data_ptr<float>() + offset, stream());
  return nblocks;
}

void clip_finalize(at::Tensor partials, long long count, double max_norm,
                   at::Tensor clip_state) {
  const char* op = "clip_finalize";
  TORCH_CHECK(partials.defined() && partials.is_cuda(), op,
              ": partials must be on the GPU");
  optim_check_f32(partials, "partials", partials.device(), op);
  optim_check_f32(clip_state, "clip_state", partials.device(), op);
  TORCH_CHECK(clip_state.numel() == 4, op,
              ": clip_state must have 4 elements, got ", clip_state.numel());
  TORCH_CHECK(count >= 0 && count <= partials.numel(), op, ": count ", count,
              " is beyond partials (", partials.numel(), " elements)");
  TORCH_CHECK(max_norm > 0.0, op, ": max_norm must be > 0 and not NaN, got ",
              max_norm);
  launch_clip_finalize(partials.data_ptr<float>(), (int)count, max_norm,
                       clip_state.data_ptr<float>(), stream());
}

void sgd_step_ext(at::Tensor p, at::Tensor g, at::Tensor m, double lr,
                  double momentum, double weight_decay, bool zero_grad,
                  c10::optional<at::Tensor> clip_state, bool decoupled) {
  const char* op = "sgd_step_ext";
  optim_check_pg(p, g, op);
  float* mptr = nullptr;
  if (m.defined() && m.numel() > 0) {
    optim_check_moment(m, "m", p, op);
    mptr = m.data_ptr<float>();
  }
  const float* cs = optim_clip_state(clip_state, p, op);
  launch_sgd_ext(is_bf16(p), p.data_ptr(), g.data_ptr(), mptr, p.numel(),
                 (float)lr, (float)momentum, (float)weight_decay,
                 zero_grad ? 1 : 0, cs, decoupled ? 1 : 0, stream());
}

void adam_step_ext(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                   double lr, double beta1, double beta2, double eps,
                   double weight_decay, double bc1, double bc2, bool zero_grad,
                   c10::optional<at::Tensor> clip_state, bool decoupled) {
  const char* op = "adam_step_ext";
  optim_check_pg(p, g, op);
  optim_check_moment(m, "m", p, op);
  optim_check_moment(v, "v", p, op);
  const float* cs = optim_clip_state(clip_state, p, op);
  launch_adam_ext(is_bf16(p), p.data_ptr(), g.data_ptr(), m.data_ptr<float>(),
                  v.data_ptr<float>(), p.numel(), (float)lr, (float)beta1,
                  (float)beta2, (float)eps, (float)weight_decay,
                  (float)(1.0 / bc1), (float)(1.0 / std::sqrt(bc2)),
                  zero_grad ? 1 : 0, cs, decoupled ? 1 : 0, stream());
}

// ---- fedmath ---------------------------------------------------------------

void scale_cast(at::Tensor dst, at::Tensor src, double alpha) {
  const char* op = "scale_cast";
  check_first(src, "src", op);
  check_vec(dst, "dst", src, "src's", at::kFloat, src.numel(), op);
  launch_scale_cast(is_bf16(src), dst.data_ptr<float>(), src.data_ptr(),
                    src.numel(), (float)alpha, stream());
}

void cast_copy(at::Tensor dst, at::Tensor src) {
  const char* op = "cast_copy";
  check_first(dst, "dst", op);
  check_vec(src, "src", dst, "dst's", at::kFloat, dst.numel(), op);
  launch_cast_copy(is_bf16(dst), dst.data_ptr(), src.data_ptr<float>(),
                   dst.numel(), stream());
}

// ---- fedopt (the federated server step) --------------------------------------
// Everything these ops refuse is refused here, before any launch, by argument
// name.

namespace {

// A buffer of a fedopt op: on the GPU (dev when given), contiguous, 16-byte
// aligned; fp32 unless any_float, n elements unless n < 0.
void fedopt_check(const at::Tensor& t, const char* name, const char* op,
                  const c10::optional<c10::Device>& dev = c10::nullopt,
                  long long n = -1, bool any_float = false) {
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on the GPU");
  TORCH_CHECK(!dev.has_value() || t.device() == *dev, op, ": ", name,
              " must be on the device of the other tensors");
  if (any_float) {
    TORCH_CHECK(
        t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, op,
        ": ", name, " must be fp32 or bf16");
  } else {
    TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name,
                " must be fp32");
  }
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ",
              name, " must be 16-byte aligned");
  TORCH_CHECK(n < 0 || t.numel() == n, op, ": ", name, " must have ", n,
              " elements, got ", t.numel());
}

int server_mode(const std::string& mode) {
  static const char* names[] = {"mean", "fedavgm", "fedadagrad", "fedadam",
                                "fedyogi"};
  for (int i = 0; i < 5; ++i)
    if (mode == names[i]) return i;
  TORCH_CHECK(false, "server_step: unknown mode '", mode,
              "' (mean, fedavgm, fedadagrad, fedadam, fedyogi)");
  return -1;
}

}  // namespace

long long delta_sumsq(at::Tensor theta, at::Tensor x, at::Tensor partials,
                      long long offset) {
  const char* op = "delta_sumsq";
  fedopt_check(theta, "theta", op, c10::nullopt, -1, true);
  fedopt_check(x, "x", op, theta.device(), theta.numel());
  fedopt_check(partials, "partials", op, theta.device());
  const long long nblocks = optim_grid(theta.numel());
  TORCH_CHECK(offset >= 0 && offset + nblocks <= partials.numel(), op,
              ": offset ", offset, " + ", nblocks, " blocks is beyond partials (",
              partials.numel(), " elements)");
  launch_delta_sumsq(is_bf16(theta), theta.data_ptr(), x.data_ptr<float>(),
                     theta.numel(), partials.data_ptr<float>() + offset,
                     stream());
  return nblocks;
}

void delta_scale_cast(at::Tensor dst, at::Tensor theta, at::Tensor x,
                      double alpha, at::Tensor clip_state,
                      c10::optional<at::Tensor> w_out) {
  const char* op = "delta_scale_cast";
  fedopt_check(theta, "theta", op, c10::nullopt, -1, true);
  fedopt_check(dst, "dst", op, theta.device(), theta.numel());
  fedopt_check(x, "x", op, theta.device(), theta.numel());
  fedopt_check(clip_state, "clip_state", op, theta.device(), 4);
  float* w = nullptr;
  if (w_out.has_value() && w_out->defined()) {
    fedopt_check(*w_out, "w_out", op, theta.device());
    TORCH_CHECK(w_out->numel() >= 1, op, ": w_out must have an element");
    w = w_out->data_ptr<float>();
  }
  TORCH_CHECK(alpha == alpha, op, ": alpha must not be NaN");
  launch_delta_scale_cast(is_bf16(theta), dst.data_ptr<float>(),
                          theta.data_ptr(), x.data_ptr<float>(), theta.numel(),
                          (float)alpha, clip_state.data_ptr<float>(), w,
                          stream());
}

void fedopt_finalize(at::Tensor w_sum, at::Tensor round_state) {
  const char* op = "fedopt_finalize";
  fedopt_check(w_sum, "w_sum", op);
  TORCH_CHECK(w_sum.numel() >= 1, op, ": w_sum must have an element");
  fedopt_check(round_state, "round_state", op, w_sum.device(), 4);
  launch_fedopt_finalize(w_sum.data_ptr<float>(),
                         round_state.data_ptr<float>(), stream());
}

namespace {

// The noise arguments of server_step_noise and dp_noise, refused by name.
struct DpNoiseArgs {
  unsigned long long seed;
  long long round, stream, elem_offset;
  double sigma;
};

void dp_noise_check(const DpNoiseArgs& nz, const char* op) {
  TORCH_CHECK(nz.round >= 0, op, ": round must be >= 0, got ", nz.round);
  TORCH_CHECK(nz.stream >= 0 && nz.stream <= 0xFFFFFFFFll, op,
              ": stream must be in [0, 2^32), got ", nz.stream);
  TORCH_CHECK(nz.elem_offset >= 0 && nz.elem_offset % 4 == 0, op,
              ": elem_offset must be a non-negative multiple of 4, got ",
              nz.elem_offset);
  TORCH_CHECK(std::isfinite(nz.sigma) && nz.sigma >= 0.0, op,
              ": sigma must be finite and >= 0, got ", nz.sigma);
}

// server_step and server_step_noise: one set of refusals, then the launch
// of NOISE = (nz != nullptr).
void server_step_impl(const char* op, const std::string& mode, at::Tensor D,
                      at::Tensor x, c10::optional<at::Tensor> m,
                      c10::optional<at::Tensor> v, double lr, double beta1,
                      double beta2, double tau, at::Tensor round_state,
                      const DpNoiseArgs* nz) {
  const int md = server_mode(mode);
  const bool has_m = md >= 1, has_v = md >= 2;
  fedopt_check(x, "x", op);
  fedopt_check(D, "D", op, x.device(), x.numel());
  float *mp = nullptr, *vp = nullptr;
  if (has_m) {
    TORCH_CHECK(m.has_value(), op, ": m is undefined (mode ", mode,
                " keeps a first moment)");
    fedopt_check(*m, "m", op, x.device(), x.numel());
    mp = m->data_ptr<float>();
  }
  if (has_v) {
    TORCH_CHECK(v.has_value(), op, ": v is undefined (mode ", mode,
                " keeps a second moment)");
    fedopt_check(*v, "v", op, x.device(), x.numel());
    vp = v->data_ptr<float>();
  }
  fedopt_check(round_state, "round_state", op, x.device(), 4);
  TORCH_CHECK(lr > 0.0, op, ": lr must be > 0 and not NaN, got ", lr);
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0, op,
              ": beta1 must be in [0, 1) and not NaN, got ", beta1);
  TORCH_CHECK(beta2 >= 0.0 && beta2 < 1.0, op,
              ": beta2 must be in [0, 1) and not NaN, got ", beta2);
  TORCH_CHECK(tau == tau, op, ": tau must not be NaN");
  TORCH_CHECK(!has_v || tau > 0.0, op,
              ": tau must be > 0 for an adaptive mode, got ", tau);
  if (nz == nullptr) {
    launch_server_step(md, D.data_ptr<float>(), x.data_ptr<float>(), mp, vp,
                       x.numel(), (float)lr, (float)beta1, (float)beta2,
                       (float)tau, round_state.data_ptr<float>(), stream());
    return;
  }
  dp_noise_check(*nz, op);
  launch_server_step_noise(
      md, D.data_ptr<float>(), x.data_ptr<float>(), mp, vp, x.numel(),
      (float)lr, (float)beta1, (float)beta2, (float)tau,
      round_state.data_ptr<float>(), nz->seed,
      (unsigned)(nz->round & 0xFFFFFFFFll), (unsigned)nz->stream,
      nz->elem_offset, (float)nz->sigma, stream());
}

}  // namespace

void server_step(const std::string& mode, at::Tensor D, at::Tensor x,
                 c10::optional<at::Tensor> m, c10::optional<at::Tensor> v,
                 double lr, double beta1, double beta2, double tau,
                 at::Tensor round_state) {
  server_step_impl("server_step", mode, D, x, m, v, lr, beta1, beta2, tau,
                   round_state, nullptr);
}

// server_step with DP-FedAvg noise (fed/server_opt.py): Delta = D + xi.
void server_step_noise(const std::string& mode, at::Tensor D, at::Tensor x,
                       c10::optional<at::Tensor> m,
                       c10::optional<at::Tensor> v, double lr, double beta1,
                       double beta2, double tau, at::Tensor round_state,
                       unsigned long long seed, long long round,
                       long long stream_id, long long elem_offset,
                       double sigma) {
  const DpNoiseArgs nz{seed, round, stream_id, elem_offset, sigma};
  server_step_impl("server_step_noise", mode, D, x, m, v, lr, beta1, beta2,
                   tau, round_state, &nz);
}

// out = xi alone: what server_step_noise adds to D, for tests and benchmarks.
void dp_noise(at::Tensor out, unsigned long long seed, long long round,
              long long stream_id, long long elem_offset, double sigma) {
  const char* op = "dp_noise";
  fedopt_check(out, "out", op);
  const DpNoiseArgs nz{seed, round, stream_id, elem_offset, sigma};
  dp_noise_check(nz, op);
  launch_dp_noise(out.data_ptr<float>(), out.numel(), seed,
                  (unsigned)(round & 0xFFFFFFFFll), (unsigned)stream_id,
                  elem_offset, (float)sigma, stream());
}

// ---- robust aggregation (fedrobust.hip) ---------------------------------------

namespace {

// K of a robust op from flags: 1 .. 16 rows.
long long robust_rows(const at::Tensor& flags, const char* op) {
  const long long K = flags.numel();
  TORCH_CHECK(K >= 1 && K <= 16, op, ": flags must have 1 to 16 elements (one "
              "per client row), got ", K);
  return K;
}

}  // namespace

// flags[K] and b_table[K + 1] -> round_state, agg_state = [k, b].
void robust_finalize(at::Tensor flags, at::Tensor b_table,
                     at::Tensor round_state, at::Tensor agg_state) {
  const char* op = "robust_finalize";
  fedopt_check(flags, "flags", op);
  const long long K = robust_rows(flags, op);
  TORCH_CHECK(b_table.defined() && b_table.is_cuda() &&
                  b_table.device() == flags.device(),
              op, ": b_table must be on the device of the other tensors");
  TORCH_CHECK(b_table.scalar_type() == at::kInt, op,
              ": b_table must be int32");
  TORCH_CHECK(b_table.is_contiguous(), op, ": b_table must be contiguous");
  TORCH_CHECK(b_table.numel() == K + 1, op, ": b_table must have ", K + 1,
              " elements (one per k = 0 .. K), got ", b_table.numel());
  fedopt_check(round_state, "round_state", op, flags.device(), 4);
  fedopt_check(agg_state, "agg_state", op, flags.device(), 2);
  launch_robust_finalize(flags.data_ptr<float>(), b_table.data_ptr<int>(),
                         (int)K, round_state.data_ptr<float>(),
                         agg_state.data_ptr<float>(), stream());
}

// D = the kept sum of the rows of U (2-D fp32, unit inner stride).
void robust_select(at::Tensor D, at::Tensor U, at::Tensor flags,
                   at::Tensor agg_state, at::Tensor round_state) {
  const char* op = "robust_select";
  fedopt_check(D, "D", op);
  TORCH_CHECK(U.defined(), op, ": U is undefined");
  TORCH_CHECK(U.is_cuda() && U.device() == D.device(), op,
              ": U must be on the device of the other tensors");
  TORCH_CHECK(U.scalar_type() == at::kFloat, op, ": U must be fp32");
  TORCH_CHECK(U.dim() == 2, op, ": U must be 2-D (K rows of n), got ", U.dim(),
              " dimensions");
  const long long K = U.size(0), n = U.size(1);
  TORCH_CHECK(K >= 1 && K <= 16, op, ": U must have 1 to 16 rows, got ", K);
  TORCH_CHECK(n == D.numel(), op, ": U's rows must have D's ", D.numel(),
              " elements, got ", n);
  TORCH_CHECK(n <= 1 || U.stride(1) == 1, op,
              ": U must have unit inner stride, got ", U.stride(1));
  const long long stride = K > 1 ? U.stride(0) : 0;
  TORCH_CHECK(stride >= 0 && (K == 1 || stride >= n), op,
              ": U's row stride ", stride, " is smaller than its row length ",
              n);
  TORCH_CHECK(stride % 4 == 0, op, ": U's row stride must be a multiple of 4 "
              "elements (16 bytes), got ", stride);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(U.data_ptr()) % 16 == 0, op,
              ": U must be 16-byte aligned");
  fedopt_check(flags, "flags", op, D.device(), K);
  fedopt_check(agg_state, "agg_state", op, D.device(), 2);
  fedopt_check(round_state, "round_state", op, D.device(), 4);
  launch_robust_select((int)K, D.data_ptr<float>(), U.data_ptr<float>(),
                       stride, n, flags.data_ptr<float>(),
                       agg_state.data_ptr<float>(),
                       round_state.data_ptr<float>(), stream());
}

at::Tensor colsum(at::Tensor x) {
  check_first(x, "x", "colsum");
  const NormShape sh = norm_shape(x, "colsum", false);
  auto out = at::zeros({sh.C}, x.options().dtype(at::kFloat));
  launch_colsum(is_bf16(x), x.data_ptr(), out.data_ptr<float>(), sh.R, sh.C,
                stream());
  return out;
}

// [R, C] -> [C, R] through the LDS tile kernel the GEMM router uses.
at::Tensor transpose2d(at::Tensor x) {
  const char* op = "transpose2d";
  check_first(x, "x", op);
  TORCH_CHECK(x.dim() == 2, op, ": x must be 2-D [R, C], got ", x.dim(), "-D");
  const long long R = x.size(0), C = x.size(1);
  TORCH_CHECK(R <= INT_MAX && C <= INT_MAX, op, ": x [", R, ", ", C,
              "] is past the kernel's int");
  auto out = at::empty({C, R}, x.options());
  if (x.numel() > 0)
    launch_transpose(is_bf16(x), x.data_ptr(), out.data_ptr(), (int)R, (int)C,
                     stream());
  return out;
}

void axpby(at::Tensor y, at::Tensor x, double a, double b) {
  const char* op = "axpby";
  TORCH_CHECK(y.defined() && y.is_cuda(), op, ": y must be on the GPU");
  TORCH_CHECK(y.scalar_type() == at::kFloat, op, ": y must be fp32");
  TORCH_CHECK(y.is_contiguous(), op, ": y must be contiguous");
  check_vec(x, "x", y, "y's", at::kFloat, y.numel(), op);
  launch_axpby(y.data_ptr<float>(), x.data_ptr<float>(), y.numel(), (float)a,
               (float)b, stream());
}

// ---- loss ------------------------------------------------------------------

// dout of a scalar loss: one fp32 element on x's device.
static void check_dout(const at::Tensor& dout, const at::Tensor& x,
                       const char* xs, const char* op) {
  check_vec(dout, "dout", x, xs, at::kFloat, 1, op);
}

at::Tensor mse_fwd(at::Tensor x, at::Tensor y) {
  const char* op = "mse_fwd";
  check_first(x, "x", op);
  check_like(y, "y", x, "x's", op, true);
  auto out = at::zeros({}, x.options().dtype(at::kFloat));
  launch_mse_fwd(is_bf16(x), x.data_ptr(), y.data_ptr(), out.data_ptr<float>(),
                 x.numel(), stream());
  launch_scale_scalar(out.data_ptr<float>(), 1.f / (float)x.numel(), stream());
  return out;
}

at::Tensor mse_bwd(at::Tensor x, at::Tensor y, at::Tensor dout) {
  const char* op = "mse_bwd";
  check_first(x, "x", op);
  check_like(y, "y", x, "x's", op, true);
  check_dout(dout, x, "x's", op);
  auto dx = at::empty_like(x);
  launch_mse_bwd(is_bf16(x), x.data_ptr(), y.data_ptr(), dout.data_ptr<float>(),
                 dx.data_ptr(), x.numel(), stream());
  return dx;
}

// logits [B, C] and the int64 labels, as ce_fwd takes them.
static void check_ce(const char* op, const at::Tensor& logits,
                     const at::Tensor& target) {
  check_first(logits, "logits", op);
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be 2-D [B, C], got ",
              logits.dim(), "-D");
  TORCH_CHECK(logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX, op,
              ": logits [", logits.size(0), ", ", logits.size(1),
              "] is past the kernels' int");
  check_vec(target, "target", logits, "the logits'", at::kLong,
            logits.size(0), op);
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target) {
  check_ce("ce_fwd", logits, target);
  int B = logits.size(0), C = logits.size(1);
  auto lse = at::empty({B}, logits.options().dtype(at::kFloat));
  auto loss = at::zeros({}, logits.options().dtype(at::kFloat));
  launch_ce_fwd(is_bf16(logits), logits.data_ptr(), reinterpret_cast<const long long*>(target.data_ptr<int64_t>()),
                lse.data_ptr<float>(), loss.data_ptr<float>(), B, C, stream());
  launch_scale_scalar(loss.data_ptr<float>(), 1.f / (float)B, stream());
  return {loss, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor dout) {
  const char* op = "ce_bwd";
  check_ce(op, logits, target);
  check_vec(lse, "lse", logits, "the logits'", at::kFloat, logits.size(0),
            op);
  check_dout(dout, logits, "the logits'", op);
  int B = logits.size(0), C = logits.size(1);
  auto dx = at::empty_like(logits);
  launch_ce_bwd(is_bf16(logits), logits.data_ptr(), reinterpret_cast<const long long*>(target.data_ptr<int64_t>()),
                lse.data_ptr<float>(), dout.data_ptr<float>(), dx.data_ptr(), B,
                C, stream());
  return dx;
}

// Cross-entropy with ignored labels (loss.hip, MASKED). Everything is refused
// here, by argument name, before anything is allocated or launched; what the
// labels hold is the kernels' business (they skip what is not a class).
static void check_ce_masked(const char* op, const at::Tensor& logits,
                            const at::Tensor& target) {
  TORCH_CHECK(logits.is_cuda(), op, ": logits must be on the GPU");
  TORCH_CHECK(logits.scalar_type() == at::kFloat ||
                  logits.scalar_type() == at::kBFloat16,
              op, ": logits must be fp32 or bf16");
  TORCH_CHECK(logits.dim() == 2, op, ": logits must be 2-D [B, C], got ",
              logits.dim(), "-D");
  TORCH_CHECK(logits.is_contiguous(), op, ": logits must be contiguous");
  TORCH_CHECK(logits.size(0) > 0 && logits.size(1) > 0, op,
              ": logits must not be empty, got [", logits.size(0), ", ",
              logits.size(1), "]");
  TORCH_CHECK(logits.size(0) <= std::numeric_limits<int>::max() &&
                  logits.size(1) <= std::numeric_limits<int>::max(),
              op, ": logits [", logits.size(0), ", ", logits.size(1),
              "] exceeds the int row / class index of the kernels");
  TORCH_CHECK(target.scalar_type() == at::kLong, op, ": target must be int64");
  TORCH_CHECK(target.is_contiguous(), op, ": target must be contiguous");
  TORCH_CHECK(target.device() == logits.device(), op,
              ": target must be on the logits' device");
  TORCH_CHECK(target.numel() == logits.size(0), op, ": target must have B = ",
              logits.size(0), " elements, got ", target.numel());
}

std::vector<at::Tensor> ce_masked_fwd(at::Tensor logits, at::Tensor target,
                                      int64_t ignore_index) {
  check_ce_masked("ce_masked_fwd", logits, target);
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto lse = at::empty({B}, logits.options().dtype(at::kFloat));
  auto loss = at::zeros({}, logits.options().dtype(at::kFloat));
  auto n_valid = at::zeros({1}, logits.options().dtype(at::kInt));
  launch_ce_masked_fwd(
      is_bf16(logits), logits.data_ptr(),
      reinterpret_cast<const long long*>(target.data_ptr<int64_t>()),
      lse.data_ptr<float>(), loss.data_ptr<float>(), n_valid.data_ptr<int>(),
      (long long)ignore_index, B, C, stream());
  return {loss, lse, n_valid};
}

at::Tensor ce_masked_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                         at::Tensor n_valid, at::Tensor dout,
                         int64_t ignore_index) {
  const char* op = "ce_masked_bwd";
  check_ce_masked(op, logits, target);
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.dim() == 1 &&
                  lse.size(0) == B && lse.is_contiguous(),
              op, ": lse must be contiguous fp32 [B = ", B, "]");
  TORCH_CHECK(lse.device() == logits.device(), op,
              ": lse must be on the logits' device");
  TORCH_CHECK(n_valid.scalar_type() == at::kInt && n_valid.numel() == 1, op,
              ": n_valid must be int32 with 1 element");
  TORCH_CHECK(n_valid.device() == logits.device(), op,
              ": n_valid must be on the logits' device");
  TORCH_CHECK(dout.scalar_type() == at::kFloat && dout.numel() == 1, op,
              ": dout must be an fp32 scalar");
  TORCH_CHECK(dout.device() == logits.device(), op,
              ": dout must be on the logits' device");
  auto dx = at::empty_like(logits);
  launch_ce_masked_bwd(
      is_bf16(logits), logits.data_ptr(),
      reinterpret_cast<const long long*>(target.data_ptr<int64_t>()),
      lse.data_ptr<float>(), n_valid.data_ptr<int>(), dout.data_ptr<float>(),
      dx.data_ptr(), (long long)ignore_index, B, C, stream());
  return dx;
}

// ---- layernorm / rmsnorm -----------------------------------------------------
// One forward and one backward for both families and their fused forms:
// center = LayerNorm (b, mean, db exist), res / plus = the fused residual add
// (z = x + res is returned after y) / residual-stream gradient (dx += plus).

static std::vector<at::Tensor> norm_rows_fwd(const char* op, bool center,
                                             const at::Tensor& x,
                                             const at::Tensor* res,
                                             const at::Tensor& w,
                                             const at::Tensor* b, double eps) {
  const NormShape sh = norm_shape(x, op, center);
  const int C = sh.C;
  const long long R = sh.R;
  if (res) norm_check_like_x(*res, "res", x, op);
  norm_check_vec(w, "w", x, x.scalar_type(), C, op);
  if (center) norm_check_vec(*b, "b", x, x.scalar_type(), C, op);
  auto y = at::empty_like(x);
  at::Tensor z = res ? at::empty_like(x) : at::Tensor();
  auto rstd = at::empty({R}, x.options().dtype(at::kFloat));
  at::Tensor mean = center ? at::empty_like(rstd) : at::Tensor();
  launch_norm_fwd(norm_row_route(R, C, is_bf16(x)), is_bf16(x), center,
                  x.data_ptr(), res ? res->data_ptr() : nullptr, w.data_ptr(),
                  center ? b->data_ptr() : nullptr, y.data_ptr(),
                  res ? z.data_ptr() : nullptr,
                  center ? mean.data_ptr<float>() : nullptr,
                  rstd.data_ptr<float>(), R, C, (float)eps, stream());
  std::vector<at::Tensor> out{y};
  if (res) out.push_back(z);
  if (center) out.push_back(mean);
  out.push_back(rstd);
  return out;
}

static std::vector<at::Tensor> norm_rows_bwd(const char* op, bool center,
                                             const at::Tensor& x,
                                             const at::Tensor& dy,
                                             const at::Tensor& w,
                                             const at::Tensor* mean,
                                             const at::Tensor& rstd,
                                             const at::Tensor* plus) {
  const NormShape sh = norm_shape(x, op, center);
  const int C = sh.C;
  const long long R = sh.R;
  norm_check_like_x(dy, "dy", x, op);
  if (plus) norm_check_like_x(*plus, "plus", x, op);
  norm_check_vec(w, "w", x, x.scalar_type(), C, op);
  if (center) norm_check_vec(*mean, "mean", x, at::kFloat, R, op);
  norm_check_vec(rstd, "rstd", x, at::kFloat, R, op);
  auto dx = at::empty_like(x);
  auto dw = at::zeros({C}, x.options().dtype(at::kFloat));
  at::Tensor db = center ? at::zeros_like(dw) : at::Tensor();
  launch_norm_bwd(norm_row_route(R, C, is_bf16(x)), is_bf16(x), center,
                  x.data_ptr(), dy.data_ptr(), w.data_ptr(),
                  center ? mean->data_ptr<float>() : nullptr,
                  rstd.data_ptr<float>(), plus ? plus->data_ptr() : nullptr,
                  dx.data_ptr(), dw.data_ptr<float>(),
                  center ? db.data_ptr<float>() : nullptr, R, C, stream());
  if (center) return {dx, dw, db};
  return {dx, dw};
}

std::vector<at::Tensor> ln_fwd(at::Tensor x, at::Tensor w, at::Tensor b,
                               double eps) {
  return norm_rows_fwd("ln_fwd", true, x, nullptr, w, &b, eps);
}
std::vector<at::Tensor> ln_add_fwd(at::Tensor x, at::Tensor res, at::Tensor w,
                                   at::Tensor b, double eps) {
  return norm_rows_fwd("ln_add_fwd", true, x, &res, w, &b, eps);
}
std::vector<at::Tensor> ln_bwd(at::Tensor x, at::Tensor dy, at::Tensor w,
                               at::Tensor mean, at::Tensor rstd) {
  return norm_rows_bwd("ln_bwd", true, x, dy, w, &mean, rstd, nullptr);
}
std::vector<at::Tensor> ln_bwd_plus(at::Tensor x, at::Tensor dy, at::Tensor w,
                                    at::Tensor mean, at::Tensor rstd,
                                    at::Tensor plus) {
  return norm_rows_bwd("ln_bwd_plus", true, x, dy, w, &mean, rstd, &plus);
}
std::vector<at::Tensor> rms_fwd(at::Tensor x, at::Tensor w, double eps) {
  return norm_rows_fwd("rms_fwd", false, x, nullptr, w, nullptr, eps);
}
std::vector<at::Tensor> rms_add_fwd(at::Tensor x, at::Tensor res, at::Tensor w,
                                    double eps) {
  return norm_rows_fwd("rms_add_fwd", false, x, &res, w, nullptr, eps);
}
std::vector<at::Tensor> rms_bwd(at::Tensor x, at::Tensor dy, at::Tensor w,
                                at::Tensor rstd) {
  return norm_rows_bwd("rms_bwd", false, x, dy, w, nullptr, rstd, nullptr);
}
std::vector<at::Tensor> rms_bwd_plus(at::Tensor x, at::Tensor dy, at::Tensor w,
                                     at::Tensor rstd, at::Tensor plus) {
  return norm_rows_bwd("rms_bwd_plus", false, x, dy, w, nullptr, rstd, &plus);
}

// ---- batchnorm (x viewed as [M, C], i.e. NHWC flattened) -------------------

std::vector<at::Tensor> bn_fwd_train(at::Tensor x, at::Tensor gamma,
                                     at::Tensor beta, at::Tensor running_mean,
                                     at::Tensor running_var, double momentum,
                                     double eps, bool relu,
                                     c10::optional<at::Tensor> res_opt) {
  at::Tensor res = res_opt.value_or(at::Tensor());
  const NormShape sh = norm_shape(x, "bn_fwd_train", false);
  const int C = sh.C;
  const long long M = sh.R;
  const bool has_res = res.defined() && res.numel() > 0;
  if (has_res) {
    norm_check_like_x(res, "res", x, "bn_fwd_train");
    TORCH_CHECK(relu, "fused residual add implies fused relu");
  }
  norm_check_vec(gamma, "gamma", x, at::kFloat, C, "bn_fwd_train");
  norm_check_vec(beta, "beta", x, at::kFloat, C, "bn_fwd_train");
  // running statistics come as a pair or not at all (empty = absent)
  const bool has_running = !norm_absent(running_mean);
  TORCH_CHECK(has_running == !norm_absent(running_var),
              "bn_fwd_train: running_mean and running_var must both be given "
              "or both be absent");
  if (has_running) {
    norm_check_vec(running_mean, "running_mean", x, at::kFloat, C,
                   "bn_fwd_train");
    norm_check_vec(running_var, "running_var", x, at::kFloat, C,
                   "bn_fwd_train");
  }
  auto sum = at::zeros({C}, x.options().dtype(at::kFloat));
  auto sumsq = at::zeros({C}, x.options().dtype(at::kFloat));
  auto mean = at::empty({C}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({C}, x.options().dtype(at::kFloat));
  auto y = at::empty_like(x);
  const BnRoute rt = bn_route(M, C, is_bf16(x));
  launch_bn_stats(rt, is_bf16(x), x.data_ptr(), sum.data_ptr<float>(),
                  sumsq.data_ptr<float>(), M, C, stream());
  float* rm = has_running ? running_mean.data_ptr<float>() : nullptr;
  float* rv = has_running ? running_var.data_ptr<float>() : nullptr;
  launch_bn_finalize(sum.data_ptr<float>(), sumsq.data_ptr<float>(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), rm, rv, M,
                     C, (float)eps, (float)momentum, stream());
  launch_bn_norm(rt, is_bf16(x), relu, x.data_ptr(),
                 has_res ? res.data_ptr() : nullptr, mean.data_ptr<float>(),
                 rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                 beta.data_ptr<float>(), y.data_ptr(), M, C, stream());
  return {y, mean, rstd};
}

at::Tensor bn_fwd_eval(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                       at::Tensor mean, at::Tensor rstd, bool relu) {
  const NormShape sh = norm_shape(x, "bn_fwd_eval", false);
  const int C = sh.C;
  const long long M = sh.R;
  norm_check_vec(gamma, "gamma", x, at::kFloat, C, "bn_fwd_eval");
  norm_check_vec(beta, "beta", x, at::kFloat, C, "bn_fwd_eval");
  norm_check_vec(mean, "mean", x, at::kFloat, C, "bn_fwd_eval");
  norm_check_vec(rstd, "rstd", x, at::kFloat, C, "bn_fwd_eval");
  auto y = at::empty_like(x);
  launch_bn_norm(bn_route(M, C, is_bf16(x)), is_bf16(x), relu, x.data_ptr(),
                 nullptr,
                 mean.data_ptr<float>(), rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                 beta.data_ptr<float>(), y.data_ptr(), M, C, stream());
  return y;
}

std::vector<at::Tensor> bn_bwd(at::Tensor x, at::Tensor dy, at::Tensor y_post,
                               at::Tensor mean, at::Tensor rstd,
                               at::Tensor gamma, bool relu, bool want_dres) {
  const NormShape sh = norm_shape(x, "bn_bwd", false);
  const int C = sh.C;
  const long long M = sh.R;
  norm_check_like_x(dy, "dy", x, "bn_bwd");
  if (relu) norm_check_like_x(y_post, "y_post", x, "bn_bwd");
  norm_check_vec(mean, "mean", x, at::kFloat, C, "bn_bwd");
  norm_check_vec(rstd, "rstd", x, at::kFloat, C, "bn_bwd");
  norm_check_vec(gamma, "gamma", x, at::kFloat, C, "bn_bwd");
  const BnRoute rt = bn_route(M, C, is_bf16(x));
  TORCH_CHECK(!want_dres || (relu && rt.dres_ok),
              "bn dres needs the fused-relu vectorized path");
  auto sum_dy = at::zeros({C}, x.options().dtype(at::kFloat));
  auto sum_dyx = at::zeros({C}, x.options().dtype(at::kFloat));
  auto dx = at::empty_like(x);
  at::Tensor dres;
  void* dres_ptr = nullptr;
  if (want_dres) {
    // fused y = relu(bn(x) + res) backward: dres = relu-masked dy, written
    // by the same dx pass. Needs the vectorized path (resnet channels).
    dres = at::empty_like(x);
    dres_ptr = dres.data_ptr();
  }
  const void* ypost_ptr = relu ? y_post.data_ptr() : x.data_ptr();
  launch_bn_bwd_stats(rt, is_bf16(x), relu, x.data_ptr(), dy.data_ptr(),
                      ypost_ptr, mean.data_ptr<float>(), rstd.data_ptr<float>(),
                      sum_dy.data_ptr<float>(), sum_dyx.data_ptr<float>(), M, C,
                      stream());
  launch_bn_bwd_dx(rt, is_bf16(x), relu, x.data_ptr(), dy.data_ptr(),
                   ypost_ptr, mean.data_ptr<float>(), rstd.data_ptr<float>(),
                   gamma.data_ptr<float>(), sum_dy.data_ptr<float>(),
                   sum_dyx.data_ptr<float>(), dx.data_ptr(), dres_ptr, M, C,
                   stream());
  // dgamma = sum_dyx, dbeta = sum_dy (fp32)
  if (want_dres) return {dx, sum_dyx, sum_dy, dres};
  return {dx, sum_dyx, sum_dy};
}

// ---- elementwise -----------------------------------------------------------

at::Tensor relu_fwd(at::Tensor x) {
  check_first(x, "x", "relu_fwd");
  auto y = at::empty_like(x);
  launch_relu_fwd(is_bf16(x), x.data_ptr(), y.data_ptr(), x.numel(), stream());
  return y;
}

at::Tensor relu_bwd(at::Tensor dy, at::Tensor y) {
  check_first(dy, "dy", "relu_bwd");
  check_like(y, "y", dy, "dy's", "relu_bwd", true);
  auto dx = at::empty_like(dy);
  launch_relu_bwd(is_bf16(dy), dy.data_ptr(), y.data_ptr(), dx.data_ptr(),
                  dy.numel(), stream());
  return dx;
}

at::Tensor add_relu_fwd(at::Tensor a, at::Tensor b) {
  check_first(a, "a", "add_relu_fwd");
  check_like(b, "b", a, "a's", "add_relu_fwd", true);
  auto y = at::empty_like(a);
  launch_add_relu_fwd(is_bf16(a), a.data_ptr(), b.data_ptr(), y.data_ptr(),
                      a.numel(), stream());
  return y;
}

at::Tensor add_scaled_fwd(at::Tensor a, at::Tensor b, double alpha) {
  check_first(a, "a", "add_scaled_fwd");
  check_like(b, "b", a, "a's", "add_scaled_fwd", true);
  auto z = at::empty_like(a);
  launch_add_scaled_fwd(is_bf16(a), a.data_ptr(), b.data_ptr(), z.data_ptr(),
                        (float)alpha, a.numel(), stream());
  return z;
}

at::Tensor scale_fwd(at::Tensor x, double alpha) {
  check_first(x, "x", "scale_fwd");
  auto z = at::empty_like(x);
  launch_scale_fwd(is_bf16(x), x.data_ptr(), z.data_ptr(), (float)alpha,
                   x.numel(), stream());
  return z;
}

at::Tensor gelu_fwd(at::Tensor x) {
  check_first(x, "x", "gelu_fwd");
  auto y = at::empty_like(x);
  launch_gelu_fwd(is_bf16(x), x.data_ptr(), y.data_ptr(), x.numel(), stream());
  return y;
}

at::Tensor gelu_bwd(at::Tensor dy, at::Tensor x) {
  check_first(dy, "dy", "gelu_bwd");
  check_like(x, "x", dy, "dy's", "gelu_bwd", true);
  auto dx = at::empty_like(dy);
  launch_gelu_bwd(is_bf16(dy), dy.data_ptr(), x.data_ptr(), dx.data_ptr(),
                  dy.numel(), stream());
  return dx;
}

// ---- gemm ------------------------------------------------------------------
// layout: 0 = NT (C=A@B^T, fwd), 1 = NN (C=A@B, dgrad), 2 = TN (C=A^T@B, wgrad)

at::Tensor gemm(at::Tensor A, at::Tensor B, int64_t layout,
                c10::optional<at::Tensor> bias_opt, bool relu, bool out_f32,
                double alpha, double beta, c10::optional<at::Tensor> C_opt,
                bool direct = false) {
  at::Tensor bias = bias_opt.value_or(at::Tensor());
  at::Tensor C_in = C_opt.value_or(at::Tensor());
  check_compute(A, "A");
  check_compute(B, "B");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "gemm wants 2-D tensors");
  TORCH_CHECK(A.scalar_type() == B.scalar_type());
  int M, N, K;
  if (layout == 0) {        // A[M,K] @ B[N,K]^T
    M = A.size(0); K = A.size(1); N = B.size(0);
    TORCH_CHECK(B.size(1) == K, "NT shape mismatch");
  } else if (layout == 1) { // A[M,K'] @ B[K',N]
    M = A.size(0); K = A.size(1); N = B.size(1);
    TORCH_CHECK(B.size(0) == K, "NN shape mismatch");
  } else {                  // A[K,M]^T @ B[K,N]
    K = A.size(0); M = A.size(1); N = B.size(1);
    TORCH_CHECK(B.size(0) == K, "TN shape mismatch");
  }
  auto out_dtype = out_f32 ? at::kFloat : A.scalar_type();
  const float* bias_ptr = nullptr;
  if (bias.defined() && bias.numel() > 0) {
    TORCH_CHECK(bias.is_cuda() && bias.is_contiguous() &&
                    bias.scalar_type() == at::kFloat && bias.numel() == N,
                "bias must be fp32 [N] on GPU");
    bias_ptr = bias.data_ptr<float>();
  }
  const GemmProblem p{is_bf16(A), out_f32, (int)layout, M, N, K,
                      bias_ptr != nullptr, relu, alpha, beta, direct, 1, false};
  const GemmPlan pl = plan_gemm(p);
  check_supported(p, pl);
  at::Tensor C;
  if (C_in.defined() && C_in.numel() > 0) {
    // the kernels write through C_in as a dense [M, N] of the output dtype
    TORCH_CHECK(C_in.is_cuda() && C_in.is_contiguous(),
                "C_in must be a contiguous GPU tensor");
    TORCH_CHECK(C_in.dim() == 2 && C_in.size(0) == M && C_in.size(1) == N,
                "C_in must be [", M, ", ", N, "]");
    TORCH_CHECK(C_in.scalar_type() == out_dtype,
                "C_in must have the output dtype");
    C = C_in;
  } else {
    TORCH_CHECK(beta == 0.0, "beta != 0 needs C_in");
    C = at::empty({M, N}, A.options().dtype(out_dtype));
  }
  at::Tensor Au = A, Bu = B;   // operands in the plan's layout
  if (pl.transpose_a) {
    Au = at::empty({M, K}, A.options());
    launch_transpose(p.bf16, A.data_ptr(), Au.data_ptr(), K, M, stream());
  }
  if (pl.transpose_b) {
    Bu = at::empty({N, K}, B.options());
    launch_transpose(p.bf16, B.data_ptr(), Bu.data_ptr(), K, N, stream());
  }
  switch (pl.kind) {
    case GemmKind::G9Slab:
    case GemmKind::G8Slab:
      run_slab(pl, Au, Bu, C, M, N, K);
      return C;
    case GemmKind::TwoPhaseSplitK: {
      auto C32 = (out_dtype == at::kFloat)
                     ? C.zero_()
                     : at::zeros({M, N}, A.options().dtype(at::kFloat));
      run_splitk(pl, Au, Bu, C32, M, N, K);
      if (out_dtype != at::kFloat)
        launch_cast_copy(true, C.data_ptr(), C32.data_ptr<float>(), C.numel(),
                         stream());
      return C;
    }
    default:
      run_dense(p, pl, Au.data_ptr(), Bu.data_ptr(), C.data_ptr(), bias_ptr);
      return C;
  }
}

// The plan gemm() (or, with batched, gemm_batched() / bmm_strided()) would
// execute for a problem, as a plain dict: routing is checkable on a machine
// with no GPU. A combination the entry points refuse raises here too.
py::dict gemm_plan(int64_t M, int64_t N, int64_t K, int64_t layout, bool bf16,
                   bool out_f32, bool has_bias, bool relu, double alpha,
                   double beta, bool direct, int64_t nbatch, bool strided,
                   bool batched) {
  const GemmProblem p{bf16, out_f32, (int)layout, (int)M, (int)N, (int)K,
                      has_bias, relu, alpha, beta, direct, (int)nbatch,
                      strided};
  const GemmPlan pl = batched ? plan_dense(p) : plan_gemm(p);
  check_supported(p, pl);   // raises what the entry points would raise
  using namespace py::literals;
  auto to_dict = [](const GemmPlan& q) {
    return py::dict(
        "transpose_a"_a = q.transpose_a, "transpose_b"_a = q.transpose_b,
        "layout"_a = q.layout, "kind"_a = kGemmKindName[(int)q.kind],
        "tile"_a = py::make_tuple(q.bm, q.bn),
        "grid"_a = py::make_tuple(q.grid_x, q.grid_y, q.grid_z),
        "splits"_a = q.splits, "k_chunk"_a = q.k_chunk,
        "use_swz"_a = q.use_swz, "m_main"_a = q.m_main);
  };
  py::dict d = to_dict(pl);
  if (pl.m_main < p.M)
    d["remainder"] = to_dict(plan_dense(gemm_remainder(p, pl)));
  else
    d["remainder"] = py::none();
  return d;
}

// ---- conv ------------------------------------------------------------------
// x: [N,H,W,Cin] NHWC contiguous; w: [Cout,KH,KW,Cin]; y: [N,HO,WO,Cout]

at::Tensor conv_fwd(at::Tensor x, at::Tensor w, int64_t stride, int64_t pad) {
  check_compute(x, "x");
  check_compute(w, "w");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4);
  int N = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
  int Cout = w.size(0), KH = w.size(1), KW = w.size(2);
  TORCH_CHECK(w.size(3) == Cin, "conv channel mismatch");
  const ConvProblem p{ConvOp::Fwd, is_bf16(x), N, H, W, Cin, Cout, KH, KW,
                      (int)stride, (int)pad};
  const ConvRoute rt = conv_route(p);
  auto y = at::empty({N, rt.HO, rt.WO, Cout}, x.options());
  bool ok = false;
  switch (rt.kind) {
    case ConvKind::Halo: {
      // fragment-ordered weight image: one wave B-load = contiguous 1 KiB
      auto wf = w.view({Cout / 16, 16, 9, Cin / 32, 4, 8})
                    .permute({2, 3, 0, 4, 1, 5}).contiguous();
      ok = launch_conv_halo(rt, p, x.data_ptr(), wf.data_ptr(), y.data_ptr(),
                            stream());
      break;
    }
    case ConvKind::Conv8:
      ok = launch_conv_8ph(rt, p, x.data_ptr(), w.data_ptr(), y.data_ptr(),
                           stream());
      break;
    default:
      ok = launch_conv_fwd(rt, p, x.data_ptr(), w.data_ptr(), y.data_ptr(),
                           stream());
  }
  check_launched(ok, p, rt);
  return y;
}

at::Tensor conv_dgrad(at::Tensor dy, at::Tensor w, int64_t H, int64_t W,
                      int64_t stride, int64_t pad) {
  check_compute(dy, "dy");
  check_compute(w, "w");
  int N = dy.size(0), Cout = w.size(0), KH = w.size(1), KW = w.size(2),
      Cin = w.size(3);
  // transposed weight copy [Cin,KH,KW,Cout]: the dgrad B operand becomes a
  // plain k-contiguous row-major matrix (glds-stageable); the permute of a
  // <= few-MB tensor is microseconds
  auto wt = w.permute({3, 1, 2, 0}).contiguous();
  auto dx = at::empty({N, H, W, Cin}, dy.options());
  const ConvProblem p{ConvOp::Dgrad, is_bf16(dy), N, (int)H, (int)W, Cin, Cout,
                      KH, KW, (int)stride, (int)pad};
  const ConvRoute rt = conv_route(p);
  bool ok = false;
  switch (rt.kind) {
    case ConvKind::Halo: {
      auto wf = wt.view({Cin / 16, 16, 9, Cout / 32, 4, 8})
                    .permute({2, 3, 0, 4, 1, 5}).contiguous();
      ok = launch_conv_halo(rt, p, dy.data_ptr(), wf.data_ptr(), dx.data_ptr(),
                            stream());
      break;
    }
    case ConvKind::Conv8:
      ok = launch_conv_8ph(rt, p, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(),
                           stream());
      break;
    default:
      ok = launch_conv_dgrad(rt, p, dy.data_ptr(), wt.data_ptr(),
                             dx.data_ptr(), stream());
  }
  check_launched(ok, p, rt);
  return dx;
}

at::Tensor conv_wgrad(at::Tensor dy, at::Tensor x, int64_t KH, int64_t KW,
                      int64_t stride, int64_t pad, bool out_f32) {
  check_compute(dy, "dy");
  check_compute(x, "x");
  int N = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
  int Cout = dy.size(3);
  // split-K accumulates in fp32 (zero-init); cast down only if requested.
  long long P = (long long)dy.size(0) * dy.size(1) * dy.size(2);
  auto dw32 = at::zeros({Cout, KH, KW, Cin}, x.options().dtype(at::kFloat));
  const ConvProblem p{ConvOp::Wgrad, is_bf16(x), N, H, W, Cin, Cout, (int)KH,
                      (int)KW, (int)stride, (int)pad};
  const ConvRoute rt = conv_route(p);
  TORCH_CHECK(P == (long long)N * rt.HO * rt.WO, "conv_wgrad: dy has ", P,
              " pixels, the conv gives ", (long long)N * rt.HO * rt.WO);
  // every route but the pixel-major one wants dy transposed once ([P,Cout]
  // -> [Cout,P]) so the wgrad A operand stages direct/glds (k = pixel
  // contiguous)
  at::Tensor dyt;
  if (rt.transpose_dy) {
    dyt = at::empty({(long long)Cout, P}, dy.options());
    launch_transpose(is_bf16(dy), dy.data_ptr(), dyt.data_ptr(), P, Cout,
                     stream());
  }
  switch (rt.kind) {
    case ConvKind::WgradPx:
      check_launched(launch_conv_wgrad_px(rt, p, dy.data_ptr(), x.data_ptr(),
                                          dw32.data_ptr(), stream()),
                     p, rt);
      break;
    case ConvKind::Wgrad1x1Slab: {
      // dw[Cout,Cin] = dy_t[Cout,P] @ x_t[Cin,P]^T on the 8-wave slab kernel
      auto xt = at::empty({(long long)Cin, P}, x.options());
      launch_transpose(true, x.data_ptr(), xt.data_ptr(), P, Cin, stream());
      run_slab(rt.gemm, dyt, xt, dw32, Cout, Cin, (int)P);
      break;
    }
    case ConvKind::Wgrad1x1SplitK:
      // dw[Cout,Cin] = dy_t[Cout,P] @ x[P,Cin], NN split-K
      run_splitk(rt.gemm, dyt, x, dw32, Cout, Cin, (int)P);
      break;
    default:
      check_launched(launch_conv_wgrad(rt, p, dyt.data_ptr(), x.data_ptr(),
                                       dw32.data_ptr(), stream()),
                     p, rt);
  }
  if (out_f32 || x.scalar_type() == at::kFloat) return dw32;
  auto dw = at::empty({Cout, KH, KW, Cin}, x.options());
  launch_cast_copy(true, dw.data_ptr(), dw32.data_ptr<float>(), dw.numel(),
                   stream());
  return dw;
}

// The route conv_fwd() / conv_dgrad() / conv_wgrad() would execute for a
// problem, as a plain dict: routing is checkable on a machine with no GPU.
py::dict conv_route_py(const std::string& op, int64_t N, int64_t H, int64_t W,
                       int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                       int64_t stride, int64_t pad, bool bf16) {
  using namespace py::literals;
  int o = -1;
  for (int i = 0; i < 3; ++i)
    if (op == kConvOpName[i]) o = i;
  TORCH_CHECK(o >= 0, "conv_route: op must be fwd, dgrad or wgrad");
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 &&
                  KW > 0 && stride > 0 && pad >= 0,
              "conv_route: bad shape");
  const ConvProblem p{(ConvOp)o, bf16, (int)N, (int)H, (int)W, (int)Cin,
                      (int)Cout, (int)KH, (int)KW, (int)stride, (int)pad};
  TORCH_CHECK(H + 2 * pad >= KH && W + 2 * pad >= KW,
              "conv_route: kernel larger than the padded image");
  const ConvRoute rt = conv_route(p);
  return py::dict(
      "kind"_a = kConvKindName[(int)rt.kind],
      "out_hw"_a = py::make_tuple(rt.HO, rt.WO),
      "tile"_a = py::make_tuple(rt.bm, rt.bn), "fast"_a = rt.fast,
      "grid"_a = py::make_tuple(rt.grid_x, rt.grid_y, rt.grid_z),
      "splits"_a = rt.splits, "p_chunk"_a = rt.p_chunk,
      "use_swz"_a = rt.use_swz, "transpose_dy"_a = rt.transpose_dy,
      "transpose_x"_a = rt.transpose_x,
      // the GEMM kernel of the 1x1 wgrad routes (gemm_plan.h), else None
      "gemm_kind"_a = (rt.kind == ConvKind::Wgrad1x1SplitK ||
                       rt.kind == ConvKind::Wgrad1x1Slab)
                          ? py::object(py::str(kGemmKindName[(int)rt.gemm.kind]))
                          : py::object(py::none()));
}


// What norm_route.h decides for [rows, C]: family "ln" / "rms" (rows = R) or
// "bn" (rows = M). The norm ops above launch exactly this.
py::dict norm_route_py(const std::string& family, int64_t rows, int64_t C,
                       bool bf16) {
  using namespace py::literals;
  TORCH_CHECK(family == "ln" || family == "rms" || family == "bn",
              "norm_route: family must be ln, rms or bn");
  TORCH_CHECK(rows > 0 && C > 0 && C <= INT_MAX, "norm_route: bad shape");
  if (family != "bn") {
    const NormRowRoute rt = norm_row_route(rows, (int)C, bf16);
    return py::dict("vec"_a = rt.vec, "trips"_a = rt.trips, "grid"_a = rt.grid,
                    "capped"_a = rt.capped, "chunks"_a = rt.chunks,
                    "rows_per_block"_a = rt.rows_per_block,
                    "grid_y"_a = rt.grid_y,
                    "direct_store"_a = rt.direct_store);
  }
  const BnRoute rt = bn_route(rows, (int)C, bf16);
  return py::dict(
      "stats"_a = rt.stats_vec ? "vec" : "scalar", "chunks"_a = rt.chunks,
      "rows_per_block"_a = rt.rows_per_block, "grid_y"_a = rt.grid_y,
      "norm"_a = rt.norm_vec ? "vec" : "scalar", "norm_trips"_a = rt.norm_trips,
      "dx"_a = rt.dx_vec ? "vec" : "scalar", "dx_trips"_a = rt.dx_trips,
      "dres_ok"_a = rt.dres_ok, "elem_grid"_a = rt.elem_grid,
      "norm_lds"_a = rt.norm_lds, "dx_lds"_a = rt.dx_lds);
}

// The index maps of the pixel-major 3x3 wgrad (wgrad_px_map.h) for one
// k-step, as plain lists: checkable on a machine with no GPU. The kernel
// calls the same functions.
py::dict wgrad_px_map(int64_t N, int64_t H, int64_t W, int64_t step) {
  using namespace py::literals;
  TORCH_CHECK(wgpx::eligible(true, (int)N, (int)H, (int)W, 64, 64, 3, 3, 1, 1),
              "wgrad_px_map: shape not eligible");
  const wgpx::Geom g = wgpx::make_geom((int)H, (int)W);
  const long long p0 = step * wgpx::PXK;
  TORCH_CHECK(step >= 0 && p0 < N * H * W, "wgrad_px_map: step out of range");
  const int h0 = (int)((p0 / W) % H);
  const int passes = wgpx::passes_of((int)W);
  // staging: chunk c = pass * THREADS + thread -> byte 16 c of the buffer
  py::list stage, window, dy_rows;
  for (int i = 0; i < wgpx::PXK; ++i) dy_rows.append(py::none());
  for (int i = 0; i < g.slots; ++i) window.append(py::none());
  for (int c = 0; c < passes * wgpx::THREADS; ++c) {
    const wgpx::ChunkSrc cs = wgpx::chunk_src(g, c);
    const bool ok = cs.kind == 1 ||
                    (cs.kind == 2 && wgpx::x_row_valid(g, h0, cs.hrel));
    const long long px = ok ? p0 + cs.rel : -1;   // flat source pixel
    stage.append(py::make_tuple(c / wgpx::THREADS, c % wgpx::THREADS, 16 * c,
                                ok ? cs.kind : 0, px, cs.sub));
    const int row = c / wgpx::CPR;
    if (c % wgpx::CPR == 0 && row < wgpx::PXK) dy_rows[row] = cs.rel;
    if (c % wgpx::CPR == 0 && row >= wgpx::PXK && row < wgpx::PXK + g.slots &&
        ok)
      window[row - wgpx::PXK] = py::make_tuple(
          px / (H * W), (px / W) % H, px % W);
  }
  py::list kpix, a_addr, b_addr;
  for (int k = 0; k < wgpx::PXK; ++k)
    kpix.append(wgpx::lin_pixel((int)W, wgpx::kslot_lin(k)));
  for (int r = 0; r < 2; ++r) {
    py::list la;
    for (int l = 0; l < 64; ++l) la.append(wgpx::a_read_addr(l, r));
    a_addr.append(la);
  }
  for (int t = 0; t < 9; ++t) {
    py::list lt;
    for (int r = 0; r < 2; ++r) {
      py::list lb;
      for (int l = 0; l < 64; ++l)
        lb.append(wgpx::b_read_addr(g, l, r) +
                  wgpx::tap_off(g, t / 3, t % 3) * wgpx::ROWB);
      lt.append(lb);
    }
    b_addr.append(lt);
  }
  return py::dict(
      "row_bytes"_a = wgpx::ROWB, "dy_rows_base"_a = 0,
      "window_base"_a = wgpx::PXK * wgpx::ROWB, "pitch"_a = g.pitch,
      "window_rows"_a = g.wrows, "slots"_a = g.slots, "passes"_a = passes,
      "threads"_a = wgpx::THREADS, "buffer_bytes"_a = passes * wgpx::THREADS * 16,
      "claimed_conflict_degree"_a = 1, "stage"_a = stage, "window"_a = window,
      "dy_rows"_a = dy_rows, "kslot_pixel"_a = kpix, "a_addr"_a = a_addr,
      "b_addr"_a = b_addr);
}

bool wgrad_px_eligible(bool bf16, int64_t N, int64_t H, int64_t W, int64_t Cin,
                       int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                       int64_t pad) {
  return wgpx::eligible(bf16, (int)N, (int)H, (int)W, (int)Cin, (int)Cout,
                        (int)KH, (int)KW, (int)stride, (int)pad);
}

py::tuple wgrad_px_split(int64_t N, int64_t H, int64_t W, int64_t Cin,
                         int64_t Cout) {
  const long long steps = N * H * W / wgpx::PXK;
  const int sps = wgpx::steps_per_split(
      steps, (int)(Cin / wgpx::TILE) * (int)(Cout / wgpx::TILE));
  return py::make_tuple(steps, sps, (steps + sps - 1) / sps);
}


// The phase map of the stride-2 dgrad (dgrad_phase_map.h) as plain lists:
// checkable on a machine with no GPU. The kernel calls the same functions.
// "classes" is in grid order; "rows" gives each class row's (n, h, w),
// "blocks" each block's (class, M tile within the class, N tile) for a
// grid of n_tiles N tiles, with or without the XCD remap.
py::dict dgrad_phase_map(int64_t N, int64_t H, int64_t W, int64_t KH,
                         int64_t KW, int64_t stride, int64_t pad, int64_t BM,
                         int64_t n_tiles, bool swz) {
  using namespace py::literals;
  TORCH_CHECK(N > 0 && H > 0 && W > 0 && BM > 0 && n_tiles > 0 &&
                  dgph::eligible((int)N, (int)H, (int)W, 32, (int)KH, (int)KW,
                                 (int)stride, (int)pad, 32),
              "dgrad_phase_map: shape not eligible");
  const dgph::Map m = dgph::make_map((int)N, (int)H, (int)W, (int)KH, (int)KW,
                                     (int)pad, (int)BM);
  py::list classes;
  for (int i = 0; i < dgph::NCLS; ++i) {
    const dgph::Class& c = m.cls[i];
    py::list taps, rows;
    for (int t = c.tap0; t < c.tap0 + c.ntaps; ++t)
      taps.append(py::make_tuple((int)m.taps[t].kh, (int)m.taps[t].kw,
                                 (int)m.taps[t].dh, (int)m.taps[t].dw));
    for (int r = 0; r < c.rows; ++r) {
      const dgph::RowPos p = dgph::row_pos(c, r);
      const int px = dgph::row_pixel(m, c, r);
      TORCH_CHECK(px == (p.n * (int)H + 2 * p.a + c.ph) * (int)W + 2 * p.b + c.pw);
      rows.append(py::make_tuple(px / (int)(H * W), (px / (int)W) % (int)H,
                                 px % (int)W));
    }
    classes.append(py::dict("ph"_a = c.ph, "pw"_a = c.pw, "Hc"_a = c.Hc,
                            "Wc"_a = c.Wc, "rows"_a = rows, "n_rows"_a = c.rows,
                            "tile0"_a = c.tile0, "tiles"_a = c.tiles,
                            "taps"_a = taps));
  }
  py::list blocks;
  for (int b = 0; b < m.m_tiles * (int)n_tiles; ++b) {
    const dgph::Tile t = dgph::block_tile(m, b, (int)n_tiles, swz ? 1 : 0);
    blocks.append(py::make_tuple(t.cls, t.m_tile, t.n_tile));
  }
  return py::dict("BM"_a = m.BM, "m_tiles"_a = m.m_tiles, "classes"_a = classes,
                  "blocks"_a = blocks);
}

// Strided batched GEMM over tensor VIEWS: operands may be non-contiguous
// slices of [B, S, h, dh] / [B, S, 3, h, dh] tensors (the attention path
// consumes them in place — no permute copies). Layouts as gemm(); all
// strides in ELEMENTS. z = outer * heads + head; B-operand head index is
// divided by b_group (GQA). C may be a preallocated strided view.
at::Tensor bmm_strided(at::Tensor A, at::Tensor B, c10::optional<at::Tensor> C_in,
                       int64_t layout, int64_t M, int64_t N, int64_t K,
                       int64_t nbatch, int64_t heads, int64_t b_group,
                       double alpha,
                       int64_t saO, int64_t saI, int64_t lda,
                       int64_t sbO, int64_t sbI, int64_t ldb,
                       int64_t scO, int64_t scI, int64_t ldc) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "bmm_strided: GPU tensors required");
  TORCH_CHECK(A.scalar_type() == B.scalar_type());
  TORCH_CHECK(A.scalar_type() == at::kFloat || A.scalar_type() == at::kBFloat16);
  const bool own_c = !(C_in.has_value() && C_in->defined());
  if (own_c) {
    scO = (int64_t)heads * M * N;
    scI = (int64_t)M * N;
    ldc = N;
  }
  GemmStrides gs{lda, ldb, ldc, (int)heads, saI, sbI, scI};
  const GemmProblem p{is_bf16(A), false, (int)layout, (int)M, (int)N, (int)K,
                      false, false, alpha, 0.0, true, (int)nbatch,
                      gs.heads > 1 || gs.lda || gs.ldb || gs.ldc};
  const GemmPlan pl = plan_dense(p);
  check_supported(p, pl);
  at::Tensor C;
  if (own_c) {
    C = at::empty({nbatch, M, N}, A.options());
  } else {
    C = *C_in;
    TORCH_CHECK(C.is_cuda() && C.scalar_type() == A.scalar_type());
  }
  run_dense(p, pl, A.data_ptr(), B.data_ptr(), C.data_ptr(), nullptr, saO, sbO,
            scO, (int)b_group, gs);
  return C;
}

// ---- batched gemm + softmax (attention) ------------------------------------
// A/B/C are 3-D [nb, *, *]; layout semantics per batch as in gemm().

at::Tensor gemm_batched(at::Tensor A, at::Tensor B, int64_t layout,
                        bool out_f32, double alpha, int64_t b_group) {
  check_compute(A, "A");
  check_compute(B, "B");
  TORCH_CHECK(A.dim() == 3 && B.dim() == 3, "gemm_batched wants 3-D tensors");
  TORCH_CHECK(A.size(0) == B.size(0) * b_group, "batch/group mismatch");
  int nb = A.size(0);
  int M, N, K;
  if (layout == 0) {
    M = A.size(1); K = A.size(2); N = B.size(1);
    TORCH_CHECK(B.size(2) == K);
  } else if (layout == 1) {
    M = A.size(1); K = A.size(2); N = B.size(2);
    TORCH_CHECK(B.size(1) == K);
  } else {
    K = A.size(1); M = A.size(2); N = B.size(2);
    TORCH_CHECK(B.size(1) == K);
  }
  const GemmProblem p{is_bf16(A), out_f32, (int)layout, M, N, K, false, false,
                      alpha, 0.0, true, nb, false};
  const GemmPlan pl = plan_dense(p);
  check_supported(p, pl);
  auto C = at::empty({nb, M, N},
                     A.options().dtype(out_f32 ? at::kFloat : A.scalar_type()));
  run_dense(p, pl, A.data_ptr(), B.data_ptr(), C.data_ptr(), nullptr,
            (long long)A.size(1) * A.size(2), (long long)B.size(1) * B.size(2),
            (long long)M * N, (int)b_group);
  return C;
}

// Per-sequence lengths of right-padded batches: an int32, contiguous tensor
// of `count` elements on `like`'s device. The values stay on the device (the
// kernels clamp them into range); only the tensor's metadata is checked.
static const int* check_lens(const c10::optional<at::Tensor>& lens,
                             const char* name, const at::Tensor& like,
                             int64_t count, const char* count_name) {
  if (!lens.has_value()) return nullptr;
  const at::Tensor& t = *lens;
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32, got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.device() == like.device(), name, " must be on ",
              like.device(), " with the other arguments, got ", t.device());
  TORCH_CHECK(t.numel() == count, name, " must have exactly ", count_name,
              " = ", count, " elements, got ", t.numel());
  return t.data_ptr<int>();
}

at::Tensor softmax_fwd(at::Tensor x, double scale, int64_t causal_seq,
                       c10::optional<at::Tensor> kv_len, int64_t rows_per_len,
                       int64_t q_period) {
  check_compute(x, "x");
  int C = x.size(-1);
  // the causal mask keeps columns c <= r % causal_seq of row r
  TORCH_CHECK(causal_seq >= 0 && causal_seq <= C,
              "softmax_fwd: causal_seq must be in [0, C = ", C, "], got ",
              causal_seq);
  long long R = x.numel() / C;
  const int* lens = nullptr;
  if (kv_len.has_value()) {
    // row r has entry r / rows_per_len and query position r % q_period
    TORCH_CHECK(rows_per_len > 0 && q_period > 0 &&
                    q_period <= std::numeric_limits<int>::max(),
                "softmax_fwd: kv_len needs rows_per_len > 0 and q_period > 0, "
                "got ", rows_per_len, " and ", q_period);
    TORCH_CHECK(R % rows_per_len == 0, "softmax_fwd: the row count ", R,
                " is not a multiple of rows_per_len = ", rows_per_len);
    lens = check_lens(kv_len, "kv_len", x, R / rows_per_len,
                      "rows / rows_per_len");
  }
  auto y = at::empty_like(x);
  launch_softmax_fwd(is_bf16(x), x.data_ptr(), y.data_ptr(), R, C,
                     (float)scale, (int)causal_seq, lens,
                     (long long)rows_per_len, (int)q_period, stream());
  return y;
}

at::Tensor softmax_bwd(at::Tensor y, at::Tensor dy, double scale) {
  check_compute(y, "y");
  check_compute(dy, "dy");
  int C = y.size(-1);
  long long R = y.numel() / C;
  auto dx = at::empty_like(y);
  launch_softmax_bwd(is_bf16(y), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), R,
                     C, (float)scale, stream());
  return dx;
}


// ---- llama ops -------------------------------------------------------------

// cos_t / sin_t: contiguous fp32 [rows >= S, D / 2] on x's device.
static void check_rope_table(const at::Tensor& t, const char* name,
                             const at::Tensor& x, long long S, long long half) {
  const char* op = "rope";
  TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), op, ": ", name,
              " must be on x's device");
  TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be fp32");
  TORCH_CHECK(t.dim() == 2, op, ": ", name, " must be 2-D [rows, D / 2], got ",
              t.dim(), "-D");
  TORCH_CHECK(t.size(0) >= S && t.size(1) == half, op, ": ", name,
              " must have at least S = ", S, " rows and exactly D / 2 = ", half,
              " columns, got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

at::Tensor rope(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t,
                bool inverse) {
  const char* op = "rope";
  check_first(x, "x", op);
  TORCH_CHECK(x.dim() == 4, op, ": x must be 4-D [B, S, H, D], got ", x.dim(),
              "-D");
  const long long S = x.size(1), H = x.size(2), D = x.size(3);
  TORCH_CHECK(D > 0 && D % 2 == 0, op, ": x must have an even D > 0, got ", D);
  TORCH_CHECK(S <= INT_MAX && H <= INT_MAX && D <= INT_MAX, op,
              ": x has S, H or D past the kernel's int");
  check_rope_table(cos_t, "cos_t", x, S, D / 2);
  check_rope_table(sin_t, "sin_t", x, S, D / 2);
  TORCH_CHECK(sin_t.sizes() == cos_t.sizes(), op,
              ": sin_t must have cos_t's sizes ", cos_t.sizes(), ", got ",
              sin_t.sizes());
  auto y = at::empty_like(x);
  long long total = x.numel() / 2;
  if (total > 0)
    launch_rope(is_bf16(x), inverse, x.data_ptr(), y.data_ptr(),
                cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), total, (int)S,
                (int)H, (int)D, stream());
  return y;
}

at::Tensor silu_mul_fwd(at::Tensor a, at::Tensor b) {
  check_first(a, "a", "silu_mul_fwd");
  check_like(b, "b", a, "a's", "silu_mul_fwd", true);
  auto y = at::empty_like(a);
  launch_silu_mul_fwd(is_bf16(a), a.data_ptr(), b.data_ptr(), y.data_ptr(),
                      a.numel(), stream());
  return y;
}

std::vector<at::Tensor> silu_mul_bwd(at::Tensor dy, at::Tensor a, at::Tensor b) {
  check_first(dy, "dy", "silu_mul_bwd");
  check_like(a, "a", dy, "dy's", "silu_mul_bwd", true);
  check_like(b, "b", dy, "dy's", "silu_mul_bwd", true);
  auto da = at::empty_like(a);
  auto db = at::empty_like(b);
  launch_silu_mul_bwd(is_bf16(a), dy.data_ptr(), a.data_ptr(), b.data_ptr(),
                      da.data_ptr(), db.data_ptr(), a.numel(), stream());
  return {da, db};
}

// ---- flash attention -------------------------------------------------------

namespace {
// The problem of 4-D views in kFlashViewName order: q, k, v[, o[, dout, dq,
// dk, dv]]. Sizes are q's, the kv head count is k's.
FlashProblem flash_problem(std::initializer_list<const at::Tensor*> views,
                           bool causal, bool varlen) {
  const at::Tensor& q = **views.begin();
  FlashProblem p{};
  p.B = q.size(0), p.S = q.size(1), p.H = q.size(2), p.DH = q.size(3);
  p.KVH = (*(views.begin() + 1))->size(2);
  p.causal = causal, p.varlen = varlen;
  for (const at::Tensor* t : views)
    p.view[p.nviews++] = AttnView{
        t->scalar_type() == at::kBFloat16, t->stride(0), t->stride(1),
        t->stride(2), t->stride(3),
        (int)(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16)};
  return p;
}
// What needs the tensors themselves, on every view; then the problem and its
// route, whose refusal (layout, head dim, head counts) is the error.
std::pair<FlashProblem, FlashRoute> checked_flash_problem(
    std::initializer_list<const at::Tensor*> views, bool causal, bool varlen) {
  int i = 0;
  for (const at::Tensor* t : views) {
    const char* name = kFlashViewName[i++];
    TORCH_CHECK(t->is_cuda(), name, " must be a bf16 GPU tensor");
    TORCH_CHECK(t->device() == (*views.begin())->device(), name,
                " must be on q's device");
    TORCH_CHECK(t->dim() == 4, name, " must be [B,S,h,dh]");
  }
  const FlashProblem p = flash_problem(views, causal, varlen);
  const FlashRoute rt = flash_route(p);
  TORCH_CHECK(rt.eligible, rt.refusal);
  return {p, rt};
}
// k and v against q: same batch, sequence and head_dim, one kv head count
void check_kv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
  for (int d : {0, 1, 3}) {
    TORCH_CHECK(k.size(d) == q.size(d), "k must share q's B, S and dh: k is ",
                k.sizes(), ", q is ", q.sizes());
    TORCH_CHECK(v.size(d) == q.size(d), "v must share q's B, S and dh: v is ",
                v.sizes(), ", q is ", q.sizes());
  }
  TORCH_CHECK(k.size(2) == v.size(2), "k and v must have the same head count");
}
void check_like_q(const at::Tensor& t, const char* name, const at::Tensor& q) {
  TORCH_CHECK(t.sizes() == q.sizes(), name, " must have q's sizes ", q.sizes(),
              ", got ", t.sizes());
}
}  // namespace

// Whether the fused kernels take these q, k, v views: flash_route's answer.
bool flash_eligible(const at::Tensor& q, const at::Tensor& k,
                    const at::Tensor& v) {
  for (const at::Tensor* t : {&q, &k, &v})
    if (!t->is_cuda() || t->dim() != 4) return false;
  return flash_route(flash_problem({&q, &k, &v}, false, false)).eligible;
}

std::vector<at::Tensor> flash_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                  at::Tensor o, bool causal,
                                  c10::optional<at::Tensor> seq_lens) {
  const auto [p, rt] =
      checked_flash_problem({&q, &k, &v, &o}, causal, seq_lens.has_value());
  check_kv(q, k, v);
  check_like_q(o, "o", q);
  FlashArgs a{};
  a.seq_lens = check_lens(seq_lens, "seq_lens", q, p.B, "B");
  auto lse = at::empty({(long long)p.B * p.H, p.S},
                       q.options().dtype(at::kFloat));
  a.q = q.data_ptr(), a.k = k.data_ptr(), a.v = v.data_ptr();
  a.o = o.data_ptr(), a.lse = lse.data_ptr<float>();
  launch_flash_fwd(rt, p, a, 1.0f / std::sqrt((float)p.DH), stream());
  return {o, lse};
}

void flash_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
               at::Tensor dout, at::Tensor lse, at::Tensor dq, at::Tensor dk,
               at::Tensor dv, bool causal,
               c10::optional<at::Tensor> seq_lens) {
  const auto [p, rt] = checked_flash_problem(
      {&q, &k, &v, &o, &dout, &dq, &dk, &dv}, causal, seq_lens.has_value());
  check_kv(q, k, v);
  check_like_q(o, "o", q);
  check_like_q(dout, "dout", q);
  check_like_q(dq, "dq", q);
  // dk/dv are per-q-head [B,S,H,dh] (GQA callers group-sum)
  check_like_q(dk, "dk (per q head)", q);
  check_like_q(dv, "dv (per q head)", q);
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() &&
                  lse.scalar_type() == at::kFloat && lse.is_contiguous(),
              "lse must be a contiguous fp32 tensor on q's device");
  TORCH_CHECK(lse.dim() == 2 && lse.size(0) == (int64_t)p.B * p.H &&
                  lse.size(1) == p.S,
              "lse must be [B*H, S] = [", (int64_t)p.B * p.H, ", ", p.S,
              "], got ", lse.sizes());
  FlashArgs a{};
  a.seq_lens = check_lens(seq_lens, "seq_lens", q, p.B, "B");
  auto delta = at::empty_like(lse);
  a.q = q.data_ptr(), a.k = k.data_ptr(), a.v = v.data_ptr();
  a.o = o.data_ptr(), a.lse = lse.data_ptr<float>();
  a.dout = dout.data_ptr(), a.delta = delta.data_ptr<float>();
  a.dq = dq.data_ptr(), a.dk = dk.data_ptr(), a.dv = dv.data_ptr();
  const float scale = 1.0f / std::sqrt((float)p.DH);
  launch_flash_delta(rt, p, a, stream());
  launch_flash_bwd_dq(rt, p, a, scale, stream());
  launch_flash_bwd_dkv(rt, p, a, scale, stream());
}

// What attn_route.h decides, from plain numbers (no GPU needed). views maps a
// view name to (4 strides, base address % 16); the views not named are
// contiguous [B, S, heads, DH]. bwd adds dout, dq, dk, dv to q, k, v, o.
py::dict flash_route_py(int64_t B, int64_t S, int64_t H, int64_t KVH,
                        int64_t DH, bool bf16, bool causal, bool varlen,
                        bool bwd, const py::dict& views) {
  using namespace py::literals;
  TORCH_CHECK(B > 0 && S > 0 && H > 0 && DH > 0 && KVH >= 0 &&
                  B * H <= INT_MAX && S <= INT_MAX && DH <= INT_MAX,
              "flash_route: bad shape");
  FlashProblem p{};
  p.B = B, p.S = S, p.H = H, p.KVH = KVH, p.DH = DH;
  p.causal = causal, p.varlen = varlen;
  p.nviews = bwd ? (int)kFlashMaxViews : 4;
  for (int i = 0; i < p.nviews; ++i) {
    const int64_t heads = (i == kK || i == kV) ? KVH : H;
    p.view[i] = AttnView{bf16, S * heads * DH, heads * DH, DH, 1, 0};
    if (views.contains(kFlashViewName[i])) {
      const auto t = views[kFlashViewName[i]].cast<std::array<int64_t, 5>>();
      p.view[i] = AttnView{bf16, t[0], t[1], t[2], t[3], (int)t[4]};
    }
  }
  const FlashRoute rt = flash_route(p);
  auto grid = [](const int* g) { return py::make_tuple(g[0], g[1]); };
  return py::dict(
      "eligible"_a = rt.eligible,
      "refusal"_a = rt.eligible ? py::object(py::none())
                                : py::object(py::str(rt.refusal)),
      "G"_a = rt.G, "grid_fwd"_a = grid(rt.grid_fwd),
      "grid_delta"_a = grid(rt.grid_delta), "grid_dq"_a = grid(rt.grid_dq),
      "grid_dkv"_a = grid(rt.grid_dkv), "lds_fwd"_a = rt.lds_fwd,
      "lds_dq"_a = rt.lds_dq, "lds_dkv"_a = rt.lds_dkv);
}

py::dict softmax_route_py(int64_t rows, int64_t C, bool bf16) {
  using namespace py::literals;
  TORCH_CHECK(rows > 0 && C > 0 && C <= INT_MAX, "softmax_route: bad shape");
  const SoftmaxRoute rt = softmax_route(rows, (int)C, bf16);
  return py::dict("kernel"_a = rt.wave ? "wave" : "block", "vec"_a = rt.vec,
                  "rows_per_block"_a = rt.rows_per_block, "grid"_a = rt.grid,
                  "capped"_a = rt.capped);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("flash_fwd", &flash_fwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("causal"), py::arg("seq_lens") = py::none());
  m.def("flash_bwd", &flash_bwd, py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("dout"), py::arg("lse"), py::arg("dq"),
        py::arg("dk"), py::arg("dv"), py::arg("causal"),
        py::arg("seq_lens") = py::none());
  m.def("flash_eligible", &flash_eligible);
  m.def("flash_route", &flash_route_py, py::arg("B"), py::arg("S"),
        py::arg("H"), py::arg("KVH"), py::arg("DH"), py::arg("bf16") = true,
        py::arg("causal") = false, py::arg("varlen") = false,
        py::arg("bwd") = false, py::arg("views") = py::dict());
  m.def("softmax_route", &softmax_route_py, py::arg("rows"), py::arg("C"),
        py::arg("bf16"));
  m.def("rms_add_fwd", &rms_add_fwd);
  m.def("rms_bwd_plus", &rms_bwd_plus);
  m.def("sgd_step", &sgd_step, "fused SGD step", py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("lr"), py::arg("momentum"),
        py::arg("weight_decay"), py::arg("zero_grad") = false);
  m.def("adam_step", &adam_step, "fused Adam step", py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("bc1"), py::arg("bc2"), py::arg("zero_grad") = false);
  m.def("optim_grid", &optim_grid_py, py::arg("n"));
  m.def("grad_sumsq", &grad_sumsq, py::arg("g"), py::arg("partials"),
        py::arg("offset"));
  m.def("clip_finalize", &clip_finalize, py::arg("partials"), py::arg("count"),
        py::arg("max_norm"), py::arg("clip_state"));
  m.def("sgd_step_ext", &sgd_step_ext, py::arg("p"), py::arg("g"), py::arg("m"),
        py::arg("lr"), py::arg("momentum"), py::arg("weight_decay"),
        py::arg("zero_grad") = false, py::arg("clip_state") = py::none(),
        py::arg("decoupled") = false);
  m.def("adam_step_ext", &adam_step_ext, py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("bc1"), py::arg("bc2"), py::arg("zero_grad") = false,
        py::arg("clip_state") = py::none(), py::arg("decoupled") = false);
  m.def("delta_sumsq", &delta_sumsq, py::arg("theta"), py::arg("x"),
        py::arg("partials"), py::arg("offset"));
  m.def("delta_scale_cast", &delta_scale_cast, py::arg("dst"),
        py::arg("theta"), py::arg("x"), py::arg("alpha"),
        py::arg("clip_state"), py::arg("w_out") = py::none());
  m.def("fedopt_finalize", &fedopt_finalize, py::arg("w_sum"),
        py::arg("round_state"));
  m.def("server_step", &server_step, py::arg("mode"), py::arg("D"),
        py::arg("x"), py::arg("m"), py::arg("v"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("tau"),
        py::arg("round_state"));
  m.def("server_step_noise", &server_step_noise, py::arg("mode"),
        py::arg("D"), py::arg("x"), py::arg("m"), py::arg("v"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("tau"),
        py::arg("round_state"), py::arg("seed"), py::arg("round"),
        py::arg("stream"), py::arg("elem_offset"), py::arg("sigma"));
  m.def("dp_noise", &dp_noise, py::arg("out"), py::arg("seed"),
        py::arg("round"), py::arg("stream"), py::arg("elem_offset"),
        py::arg("sigma"));
  m.def("robust_finalize", &robust_finalize, py::arg("flags"),
        py::arg("b_table"), py::arg("round_state"), py::arg("agg_state"));
  m.def("robust_select", &robust_select, py::arg("D"), py::arg("U"),
        py::arg("flags"), py::arg("agg_state"), py::arg("round_state"));
  m.def("scale_cast", &scale_cast);
  m.def("cast_copy", &cast_copy);
  m.def("axpby", &axpby);
  m.def("bmm_strided", &bmm_strided, py::arg("A"), py::arg("B"),
        py::arg("C_in") = py::none(), py::arg("layout") = 0,
        py::arg("M") = 0, py::arg("N") = 0, py::arg("K") = 0,
        py::arg("nbatch") = 1, py::arg("heads") = 1,
        py::arg("b_group") = 1, py::arg("alpha") = 1.0,
        py::arg("saO") = 0, py::arg("saI") = 0, py::arg("lda") = 0,
        py::arg("sbO") = 0, py::arg("sbI") = 0, py::arg("ldb") = 0,
        py::arg("scO") = 0, py::arg("scI") = 0, py::arg("ldc") = 0);
  m.def("colsum", &colsum);
  m.def("transpose2d", &transpose2d);
  m.def("mse_fwd", &mse_fwd);
  m.def("mse_bwd", &mse_bwd);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_masked_fwd", &ce_masked_fwd);
  m.def("ce_masked_bwd", &ce_masked_bwd);
  m.def("ln_fwd", &ln_fwd);
  m.def("ln_bwd", &ln_bwd);
  m.def("ln_add_fwd", &ln_add_fwd);
  m.def("ln_bwd_plus", &ln_bwd_plus);
  m.def("bn_fwd_train", &bn_fwd_train, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("running_mean"), py::arg("running_var"),
        py::arg("momentum"), py::arg("eps"), py::arg("relu"),
        py::arg("res") = py::none());
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("bn_bwd", &bn_bwd, py::arg("x"), py::arg("dy"), py::arg("y_post"),
        py::arg("mean"), py::arg("rstd"), py::arg("gamma"), py::arg("relu"),
        py::arg("want_dres") = false);
  m.def("relu_fwd", &relu_fwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("add_relu_fwd", &add_relu_fwd);
  m.def("add_scaled_fwd", &add_scaled_fwd);
  m.def("scale_fwd", &scale_fwd);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("gemm", &gemm, py::arg("A"), py::arg("B"), py::arg("layout"),
        py::arg("bias") = py::none(), py::arg("relu") = false,
        py::arg("out_f32") = false, py::arg("alpha") = 1.0,
        py::arg("beta") = 0.0, py::arg("C_in") = py::none(),
        py::arg("direct") = false);
  m.def("gemm_plan", &gemm_plan, py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("layout") = 0, py::arg("bf16") = true,
        py::arg("out_f32") = false, py::arg("has_bias") = false,
        py::arg("relu") = false, py::arg("alpha") = 1.0, py::arg("beta") = 0.0,
        py::arg("direct") = false, py::arg("nbatch") = 1,
        py::arg("strided") = false, py::arg("batched") = false);
  m.def("gemm_batched", &gemm_batched, py::arg("A"), py::arg("B"),
        py::arg("layout"), py::arg("out_f32") = false, py::arg("alpha") = 1.0,
        py::arg("b_group") = 1);
  m.def("softmax_fwd", &softmax_fwd, py::arg("x"), py::arg("scale") = 1.0,
        py::arg("causal_seq") = 0, py::arg("kv_len") = py::none(),
        py::arg("rows_per_len") = 0, py::arg("q_period") = 0);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("rms_fwd", &rms_fwd);
  m.def("rms_bwd", &rms_bwd);
  m.def("rope", &rope, py::arg("x"), py::arg("cos_t"), py::arg("sin_t"),
        py::arg("inverse") = false);
  m.def("silu_mul_fwd", &silu_mul_fwd);
  m.def("silu_mul_bwd", &silu_mul_bwd);
  m.def("conv_route", &conv_route_py, py::arg("op"), py::arg("N"),
        py::arg("H"), py::arg("W"), py::arg("Cin"), py::arg("Cout"),
        py::arg("KH"), py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("bf16") = true);
  m.def("norm_route", &norm_route_py, py::arg("family"), py::arg("rows"),
        py::arg("C"), py::arg("bf16"));
  m.def("conv_fwd", &conv_fwd);
  m.def("conv_dgrad", &conv_dgrad);
  m.def("conv_wgrad", &conv_wgrad);
  m.def("dgrad_phase_map", &dgrad_phase_map, py::arg("N"), py::arg("H"),
        py::arg("W"), py::arg("KH"), py::arg("KW"), py::arg("stride"),
        py::arg("pad"), py::arg("BM"), py::arg("n_tiles") = 1,
        py::arg("swz") = false);
  m.def("wgrad_px_map", &wgrad_px_map, py::arg("N"), py::arg("H"),
        py::arg("W"), py::arg("step"));
  m.def("wgrad_px_eligible", &wgrad_px_eligible);
  m.def("wgrad_px_split", &wgrad_px_split);
}

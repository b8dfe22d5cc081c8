// torch.ops.sgrender.final_conv / final_conv_bwd: the BRDF decoders' last step, dconvFinal(dpadFinal(.)) of models.decoder0 (models.py:155-156,
// 187) -- ReplicationPad2d(1) + Conv2d(C -> 3, k = 3) -- optionally with GroupNorm + ReLU (models.py:183) as the convolution's load
// prologue, as operators of the C++ torch extension.
//
// Same rules as sgr_torch_gn_stage.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_final_conv_fwd / _bwd, sgr_gn_moments of include/sgrender.h) on the current HIP stream; nothing here
// computes and nothing synchronises.  x travels with its strides: a channels-last convolution output is not copied.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

constexpr int64_t kMaxC = 256;      // kFcMaxC of csrc/sgr_final_conv.h: the weight tile stays in LDS
constexpr const char* kCompose = "; compose F.pad(., (1, 1, 1, 1), mode='replicate') and F.conv2d (after group_norm_relu, if there is a GroupNorm) instead";

struct Conv {
  int64_t B = 0, C = 0, H = 0, W = 0, G = 0;
  bool fused = false;
};

void check_sizes(const Conv& s, int64_t O, const char* who) {
  TORCH_CHECK(s.B > 0 && s.C > 0 && s.H > 0 && s.W > 0, "sgrender: ", who, ": zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(O == 3, "sgrender: ", who, ": the convolution must have exactly 3 output channels (dconvFinal), got ", O, kCompose);
  TORCH_CHECK(s.C <= kMaxC, "sgrender: ", who, ": ", s.C, " input channels, at most ", kMaxC, " are supported", kCompose);
  TORCH_CHECK(s.B <= 65535 && s.H * s.W < (int64_t(1) << 26), "sgrender: ", who, ": size out of range");
  if (s.fused) TORCH_CHECK(s.G > 0 && s.C % s.G == 0, "sgrender: ", who, ": the channel count ", s.C, " is not a multiple of num_groups ", s.G);
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Conv check_fwd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& gnw, const OT& gnb, int64_t G, double eps, bool device) {
  TORCH_CHECK(has(gnw) == has(gnb), "sgrender: final_conv: the GroupNorm weight and bias come together or not at all");
  const bool fused = has(gnw);
  if (device) TORCH_CHECK(x.is_cuda() && weight.is_cuda() && bias.is_cuda() && (!fused || (gnw->is_cuda() && gnb->is_cuda())), kNoCpu);
  TORCH_CHECK(x.scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat &&
                  (!fused || (gnw->scalar_type() == at::kFloat && gnb->scalar_type() == at::kFloat)),
              "sgrender: final_conv: fp32 tensors required (x ", x.scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(), ")");
  TORCH_CHECK(x.dim() == 4, "sgrender: final_conv: x must be [B,C,H,W], got ", x.sizes());
  Conv s;
  s.B = x.size(0); s.C = x.size(1); s.H = x.size(2); s.W = x.size(3); s.G = G; s.fused = fused;
  TORCH_CHECK(weight.dim() == 4 && weight.size(1) == s.C && weight.size(2) == 3 && weight.size(3) == 3, "sgrender: final_conv: weight must be [3,", s.C,
              ",3,3] (a 3x3 kernel over x's channels), got ", weight.sizes(), kCompose);
  check_sizes(s, weight.size(0), "final_conv");
  TORCH_CHECK(bias.dim() == 1 && bias.size(0) == 3, "sgrender: final_conv: bias must be [3], got ", bias.sizes());
  TORCH_CHECK(weight.device() == x.device() && bias.device() == x.device(), "sgrender: final_conv: tensors on different devices");
  if (fused) {
    TORCH_CHECK(gnw->dim() == 1 && gnw->size(0) == s.C && gnb->dim() == 1 && gnb->size(0) == s.C, "sgrender: final_conv: the GroupNorm weight and bias must be [", s.C,
                "], got ", gnw->sizes(), " and ", gnb->sizes());
    TORCH_CHECK(eps > 0, "sgrender: final_conv: eps must be positive");
    TORCH_CHECK(gnw->device() == x.device() && gnb->device() == x.device(), "sgrender: final_conv: tensors on different devices");
  }
  return s;
}

// -> (out [B,3,H,W], stats [B,G,4]; [0] without a GroupNorm)
T2 final_conv_cuda(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& gnw, const OT& gnb, int64_t G, double eps) {
  const Conv s = check_fwd(x, weight, bias, gnw, gnb, G, eps, true);
  const c10::DeviceGuard guard(x.device());
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous);
  Tensor out = at::empty({s.B, 3, s.H, s.W}, o), stats = at::empty({0}, o), gw, gb;
  const Tensor w = weight.contiguous(), b = bias.contiguous();
  const Strides4 xs = strides_of(x);
  if (s.fused) {
    gw = gnw->contiguous(); gb = gnb->contiguous();
    stats = at::empty({s.B, s.G, 4}, o);
    const Tensor ws = workspace_floats(api().sgr_gn_stage_workspace_floats((int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, 0, 0), "final_conv", o);
    ok(api().sgr_gn_moments(rp(x), wp(stats), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, xs.v, (float)eps, stream_of(x.device())), "sgr_gn_moments");
  }
  ok(api().sgr_final_conv_fwd(rp(x), rp(w), rp(b), rp(gw), rp(gb), s.fused ? rp(stats) : nullptr, wp(out), (int)s.B, (int)s.C, 3, (int)s.G, (int)s.H, (int)s.W, xs.v,
                              stream_of(x.device())),
     "sgr_final_conv_fwd");
  return {out, stats};
}
T2 final_conv_meta(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& gnw, const OT& gnb, int64_t G, double eps) {
  const Conv s = check_fwd(x, weight, bias, gnw, gnb, G, eps, false);
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous);
  return {at::empty({s.B, 3, s.H, s.W}, o), s.fused ? at::empty({s.B, s.G, 4}, o) : at::empty({0}, o)};
}

// the backward's own checks.  x is needed for dweight, weight for dy; gn_weight / gn_bias / stats (all three or none) make x the GroupNorm's
// input and dy the gradient at the ReLU's output
Conv check_bwd(const Tensor& g, const OT& x, const OT& weight, const OT& gnw, const OT& gnb, const OT& stats, int64_t C, int64_t G, bool nY, bool nW, bool nB,
               bool device) {
  TORCH_CHECK(nY || nW || nB, "sgrender: final_conv_bwd: no gradient requested");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == at::kFloat && g.size(1) == 3, "sgrender: final_conv_bwd: the cotangent must be fp32 [B,3,H,W], got ", g.scalar_type(), " ",
              g.sizes());
  TORCH_CHECK(has(gnw) == has(gnb) && has(gnw) == has(stats), "sgrender: final_conv_bwd: the GroupNorm weight, bias and statistics come together or not at all");
  Conv s;
  s.B = g.size(0); s.C = C; s.H = g.size(2); s.W = g.size(3); s.G = G; s.fused = has(stats);
  check_sizes(s, 3, "final_conv_bwd");
  if (nY) {
    TORCH_CHECK(has(weight), "sgrender: final_conv_bwd: weight is needed for dy");
    if (device) TORCH_CHECK(weight->is_cuda(), kNoCpu);
    TORCH_CHECK(weight->scalar_type() == at::kFloat && weight->sizes() == at::IntArrayRef({3, s.C, 3, 3}), "sgrender: final_conv_bwd: weight must be fp32 [3,", s.C,
                ",3,3], got ", weight->scalar_type(), " ", weight->sizes());
  }
  if (nW) {
    TORCH_CHECK(has(x), "sgrender: final_conv_bwd: x is needed for dweight");
    if (device) TORCH_CHECK(x->is_cuda() && (!s.fused || (gnw->is_cuda() && gnb->is_cuda() && stats->is_cuda())), kNoCpu);
    TORCH_CHECK(x->scalar_type() == at::kFloat && x->sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: final_conv_bwd: x must be fp32 [", s.B, ",", s.C, ",", s.H,
                ",", s.W, "], got ", x->scalar_type(), " ", x->sizes());
    if (s.fused) {
      TORCH_CHECK(gnw->scalar_type() == at::kFloat && gnb->scalar_type() == at::kFloat && gnw->dim() == 1 && gnb->dim() == 1 && gnw->size(0) == s.C && gnb->size(0) == s.C,
                  "sgrender: final_conv_bwd: the GroupNorm weight and bias must be fp32 [", s.C, "]");
      TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->sizes() == at::IntArrayRef({s.B, s.G, 4}), "sgrender: final_conv_bwd: stats must be fp32 [", s.B, ",", s.G,
                  ",4], got ", stats->sizes());
    }
  }
  return s;
}
// a [0] tensor where a gradient is not wanted
T3 bwd_outputs(const Conv& s, const at::TensorOptions& o, bool nY, bool nW, bool nB) {
  return {nY ? at::empty({s.B, s.C, s.H, s.W}, o) : none(o), nW ? at::empty({3, s.C, 3, 3}, o) : none(o), nB ? at::empty({3}, o) : none(o)};
}
T3 final_conv_bwd_cuda(const Tensor& g, const OT& x, const OT& weight, const OT& gnw, const OT& gnb, const OT& stats, int64_t C, int64_t G, bool nY, bool nW, bool nB) {
  const Conv s = check_bwd(g, x, weight, gnw, gnb, stats, C, G, nY, nW, nB, true);
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  T3 out = bwd_outputs(s, o, nY, nW, nB);
  const Tensor gc = g.contiguous();
  Tensor w, gw, gb, st, ws;
  Strides4 xs{};
  if (nY) w = weight->contiguous();
  if (nW) {
    xs = strides_of(*x);
    if (s.fused) { gw = gnw->contiguous(); gb = gnb->contiguous(); st = stats->contiguous(); }
  }
  if (nW || nB) {
    ws = workspace_floats(api().sgr_final_conv_workspace_floats((int)s.B, (int)s.C, 3, (int)s.H, (int)s.W), "final_conv_bwd", o);
  }
  ok(api().sgr_final_conv_bwd(rp(gc), nW ? rp(*x) : nullptr, rp(w), rp(gw), rp(gb), rp(st), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), wp(ws),
                              (int)s.B, (int)s.C, 3, (int)s.G, (int)s.H, (int)s.W, nW ? xs.v : nullptr, stream_of(g.device())),
     "sgr_final_conv_bwd");
  return out;
}
T3 final_conv_bwd_meta(const Tensor& g, const OT& x, const OT& weight, const OT& gnw, const OT& gnb, const OT& stats, int64_t C, int64_t G, bool nY, bool nW, bool nB) {
  const Conv s = check_bwd(g, x, weight, gnw, gnb, stats, C, G, nY, nW, nB, false);
  return bwd_outputs(s, g.options().memory_format(at::MemoryFormat::Contiguous), nY, nW, nB);
}

using FwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const OT&, const OT&, int64_t, double);
using BwdSig = T3(const Tensor&, const OT&, const OT&, const OT&, const OT&, const OT&, int64_t, int64_t, bool, bool, bool);
using GnBwdSig = T4(const Tensor&, const OT&, const OT&, const OT&, const OT&, int64_t, int64_t, int64_t, bool, bool, bool, bool);

struct FinalConvFn : public torch::autograd::Function<FinalConvFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& gnw, const OT& gnb, int64_t G, double eps,
                               bool nX, bool nW, bool nB, bool nGW, bool nGB) {
    T2 out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::final_conv");
      out = op.call(x, weight, bias, gnw, gnb, G, eps);
    }
    // plain: x is y, kept for dweight.  With a GroupNorm: x, its parameters and the statistics -- y is recomputed from them, never kept
    const bool fused = has(gnw), gn_side = fused && (nX || nGW || nGB), need_y = fused ? gn_side : nX;
    const bool keep_gn = fused && (nW || gn_side);
    ctx->save_for_backward({(nW || gn_side) ? x : Tensor(), need_y ? weight : Tensor(), keep_gn ? *gnw : Tensor(), keep_gn ? *gnb : Tensor(),
                            keep_gn ? std::get<1>(out) : Tensor()});
    ctx->saved_data["C"] = x.size(1);
    ctx->saved_data["G"] = G;
    ctx->saved_data["fused"] = fused;
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB; ctx->saved_data["nGW"] = nGW; ctx->saved_data["nGB"] = nGB;
    ctx->mark_non_differentiable({std::get<1>(out)});
    return {std::get<0>(out), std::get<1>(out)};
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(12);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const bool fused = ctx->saved_data["fused"].toBool(), nX = ctx->saved_data["nX"].toBool(), nW = ctx->saved_data["nW"].toBool(), nB = ctx->saved_data["nB"].toBool(),
               nGW = ctx->saved_data["nGW"].toBool(), nGB = ctx->saved_data["nGB"].toBool();
    const bool gn_side = fused && (nX || nGW || nGB), need_y = fused ? gn_side : nX;
    const int64_t C = ctx->saved_data["C"].toInt(), G = ctx->saved_data["G"].toInt();
    static auto bwd = find_op<BwdSig>("sgrender::final_conv_bwd");
    auto [dy, dw, db] = bwd.call(g[0], nW ? opt_of(s[0]) : OT(), opt_of(s[1]), opt_of(s[2]), opt_of(s[3]), opt_of(s[4]), C, G, need_y, nW, nB);
    if (nW) out[1] = dw;
    if (nB) out[2] = db;
    if (!fused) {
      if (nX) out[0] = dy;
      return out;
    }
    if (gn_side) {      // the stage's own backward: it recomputes the ReLU's mask from x, so dy goes in unmasked
      static auto gn_bwd = find_op<GnBwdSig>("sgrender::gn_stage_bwd");
      auto [dx, dgw, dgb, ds] = gn_bwd.call(dy, opt_of(s[0]), opt_of(s[2]), opt_of(s[3]), opt_of(s[4]), C, (int64_t)0, G, nX, nGW, nGB, false);
      if (nX) out[0] = dx;
      if (nGW) out[3] = dgw;
      if (nGB) out[4] = dgb;
    }
    return out;
  }
};

T2 final_conv_autograd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& gnw, const OT& gnb, int64_t G, double eps) {
  const bool grad = at::GradMode::is_enabled();
  const bool nX = grad && x.requires_grad(), nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad();
  const bool nGW = grad && has(gnw) && gnw->requires_grad(), nGB = grad && has(gnb) && gnb->requires_grad();
  if (!(nX || nW || nB || nGW || nGB)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::final_conv");
    return op.call(x, weight, bias, gnw, gnb, G, eps);
  }
  auto o = FinalConvFn::apply(x, weight, bias, gnw, gnb, G, eps, nX, nW, nB, nGW, nGB);
  return {o[0], o[1]};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("final_conv(Tensor x, Tensor weight, Tensor bias, Tensor? gn_weight, Tensor? gn_bias, int num_groups, float eps=1e-05) -> (Tensor, Tensor)");
  m.def("final_conv_bwd(Tensor g, Tensor? x, Tensor? weight, Tensor? gn_weight, Tensor? gn_bias, Tensor? stats, int channels, int num_groups, bool need_y, "
        "bool need_weight, bool need_bias) -> (Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("final_conv", &final_conv_cuda);
  m.impl("final_conv_bwd", &final_conv_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("final_conv", &final_conv_meta);
  m.impl("final_conv_bwd", &final_conv_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("final_conv", &final_conv_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"final_conv", "final_conv_bwd"}); }

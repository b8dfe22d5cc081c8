// torch.ops.sgrender.light_final_conv / light_final_conv_bwd: the light decoders' last step, dconvFinal(dpadFinal(.)) of models.decoderLight
// (models.py:297-302, 334) -- ReplicationPad2d(1) + Conv2d(C -> O, k = 3), O = SGNum or 3 SGNum -- as operators of the C++ torch extension.
//
// Same rules as sgr_torch_final_conv.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_light_final_conv_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes
// and nothing synchronises.  y travels with its strides: a channels-last convolution output is not copied.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

constexpr int64_t kMaxO = 48, kMinC = 16, kMaxC = 256;      // kLfMaxO, kLfMinC, kLfMaxC of csrc/sgr_light_final_conv.h
constexpr const char* kCompose = "; compose F.pad(., (1, 1, 1, 1), mode='replicate') and F.conv2d instead";

struct Conv { int64_t B = 0, C = 0, O = 0, H = 0, W = 0; };

void check_sizes(const Conv& s, const char* who) {
  TORCH_CHECK(s.B > 0 && s.C > 0 && s.H > 0 && s.W > 0, "sgrender: ", who, ": zero-sized y [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.O >= 1 && s.O <= kMaxO, "sgrender: ", who, ": ", s.O, " output channels, 1..", kMaxO, " are supported", kCompose);
  TORCH_CHECK(s.C >= kMinC && s.C <= kMaxC && s.C % 16 == 0, "sgrender: ", who, ": ", s.C, " input channels, a multiple of 16 in ", kMinC, "..", kMaxC,
              " is supported", kCompose);
  TORCH_CHECK(s.B <= 65535 && s.H * s.W < (int64_t(1) << 26), "sgrender: ", who, ": size out of range", kCompose);
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Conv check_fwd(const Tensor& y, const Tensor& weight, const Tensor& bias, bool device) {
  if (device) TORCH_CHECK(y.is_cuda() && weight.is_cuda() && bias.is_cuda(), kNoCpu);
  TORCH_CHECK(y.scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat,
              "sgrender: light_final_conv: fp32 tensors required (y ", y.scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(), ")", kCompose);
  TORCH_CHECK(y.dim() == 4, "sgrender: light_final_conv: y must be [B,C,H,W], got ", y.sizes(), kCompose);
  Conv s;
  s.B = y.size(0); s.C = y.size(1); s.H = y.size(2); s.W = y.size(3);
  TORCH_CHECK(weight.dim() == 4 && weight.size(1) == s.C && weight.size(2) == 3 && weight.size(3) == 3, "sgrender: light_final_conv: weight must be [O,", s.C,
              ",3,3] (a 3x3 kernel over y's channels), got ", weight.sizes(), kCompose);
  s.O = weight.size(0);
  check_sizes(s, "light_final_conv");
  TORCH_CHECK(bias.dim() == 1 && bias.size(0) == s.O, "sgrender: light_final_conv: bias must be [", s.O, "], got ", bias.sizes(), kCompose);
  TORCH_CHECK(weight.device() == y.device() && bias.device() == y.device(), "sgrender: light_final_conv: tensors on different devices");
  return s;
}

Tensor light_final_conv_cuda(const Tensor& y, const Tensor& weight, const Tensor& bias) {
  const Conv s = check_fwd(y, weight, bias, true);
  const c10::DeviceGuard guard(y.device());
  Tensor out = at::empty({s.B, s.O, s.H, s.W}, y.options().memory_format(at::MemoryFormat::Contiguous));
  const Tensor w = weight.contiguous(), b = bias.contiguous();
  const Strides4 ys = strides_of(y);
  ok(api().sgr_light_final_conv_fwd(rp(y), rp(w), rp(b), wp(out), (int)s.B, (int)s.C, (int)s.O, (int)s.H, (int)s.W, ys.v, stream_of(y.device())),
     "sgr_light_final_conv_fwd");
  return out;
}
Tensor light_final_conv_meta(const Tensor& y, const Tensor& weight, const Tensor& bias) {
  const Conv s = check_fwd(y, weight, bias, false);
  return at::empty({s.B, s.O, s.H, s.W}, y.options().memory_format(at::MemoryFormat::Contiguous));
}

// the backward's own checks.  y is needed for dweight, weight for dy; the sizes come from whichever of the two is there
Conv check_bwd(const Tensor& g, const OT& y, const OT& weight, bool nY, bool nW, bool nB, bool device) {
  TORCH_CHECK(nY || nW || nB, "sgrender: light_final_conv_bwd: no gradient requested");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == at::kFloat, "sgrender: light_final_conv_bwd: the cotangent must be fp32 [B,O,H,W], got ", g.scalar_type(), " ", g.sizes());
  Conv s;
  s.B = g.size(0); s.O = g.size(1); s.H = g.size(2); s.W = g.size(3);
  TORCH_CHECK(!nY || has(weight), "sgrender: light_final_conv_bwd: weight is needed for dy");
  TORCH_CHECK(!nW || has(y), "sgrender: light_final_conv_bwd: y is needed for dweight");
  s.C = has(weight) ? (weight->dim() == 4 ? weight->size(1) : 0) : has(y) ? (y->dim() == 4 ? y->size(1) : 0) : kMinC;      // dbias alone: C is not used
  if (nY) {
    if (device) TORCH_CHECK(weight->is_cuda(), kNoCpu);
    TORCH_CHECK(weight->scalar_type() == at::kFloat && weight->sizes() == at::IntArrayRef({s.O, s.C, 3, 3}), "sgrender: light_final_conv_bwd: weight must be fp32 [", s.O,
                ",C,3,3], got ", weight->scalar_type(), " ", weight->sizes());
  }
  if (nW) {
    if (device) TORCH_CHECK(y->is_cuda(), kNoCpu);
    TORCH_CHECK(y->scalar_type() == at::kFloat && y->sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: light_final_conv_bwd: y must be fp32 [", s.B, ",", s.C, ",",
                s.H, ",", s.W, "], got ", y->scalar_type(), " ", y->sizes());
  }
  check_sizes(s, "light_final_conv_bwd");
  return s;
}
// a [0] tensor where a gradient is not wanted
T3 bwd_outputs(const Conv& s, const at::TensorOptions& o, bool nY, bool nW, bool nB) {
  return {nY ? at::empty({s.B, s.C, s.H, s.W}, o) : none(o), nW ? at::empty({s.O, s.C, 3, 3}, o) : none(o), nB ? at::empty({s.O}, o) : none(o)};
}
T3 light_final_conv_bwd_cuda(const Tensor& g, const OT& y, const OT& weight, bool nY, bool nW, bool nB) {
  const Conv s = check_bwd(g, y, weight, nY, nW, nB, true);
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  T3 out = bwd_outputs(s, o, nY, nW, nB);
  const Tensor gc = g.contiguous();
  Tensor w, ws;
  Strides4 ys{};
  if (nY) w = weight->contiguous();
  if (nW) ys = strides_of(*y);
  if (nW || nB) {
    ws = workspace_floats(api().sgr_light_final_conv_workspace_floats((int)s.B, (int)s.C, (int)s.O, (int)s.H, (int)s.W), "light_final_conv_bwd", o);
  }
  ok(api().sgr_light_final_conv_bwd(rp(gc), nW ? rp(*y) : nullptr, rp(w), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), wp(ws), (int)s.B, (int)s.C,
                                    (int)s.O, (int)s.H, (int)s.W, nW ? ys.v : nullptr, stream_of(g.device())),
     "sgr_light_final_conv_bwd");
  return out;
}
T3 light_final_conv_bwd_meta(const Tensor& g, const OT& y, const OT& weight, bool nY, bool nW, bool nB) {
  const Conv s = check_bwd(g, y, weight, nY, nW, nB, false);
  return bwd_outputs(s, g.options().memory_format(at::MemoryFormat::Contiguous), nY, nW, nB);
}

using FwdSig = Tensor(const Tensor&, const Tensor&, const Tensor&);
using BwdSig = T3(const Tensor&, const OT&, const OT&, bool, bool, bool);

struct LightFinalConvFn : public torch::autograd::Function<LightFinalConvFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& y, const Tensor& weight, const Tensor& bias, bool nY, bool nW, bool nB) {
    Tensor out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::light_final_conv");
      out = op.call(y, weight, bias);
    }
    // y is kept only for dweight, the weight only for dy
    ctx->save_for_backward({nW ? y : Tensor(), nY ? weight : Tensor()});
    ctx->saved_data["nY"] = nY; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(6);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const bool nY = ctx->saved_data["nY"].toBool(), nW = ctx->saved_data["nW"].toBool(), nB = ctx->saved_data["nB"].toBool();
    static auto bwd = find_op<BwdSig>("sgrender::light_final_conv_bwd");
    auto [dy, dw, db] = bwd.call(g[0], opt_of(s[0]), opt_of(s[1]), nY, nW, nB);
    if (nY) out[0] = dy;
    if (nW) out[1] = dw;
    if (nB) out[2] = db;
    return out;
  }
};

Tensor light_final_conv_autograd(const Tensor& y, const Tensor& weight, const Tensor& bias) {
  const bool grad = at::GradMode::is_enabled();
  const bool nY = grad && y.requires_grad(), nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad();
  if (!(nY || nW || nB)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::light_final_conv");
    return op.call(y, weight, bias);
  }
  return LightFinalConvFn::apply(y, weight, bias, nY, nW, nB);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("light_final_conv(Tensor y, Tensor weight, Tensor bias) -> Tensor");
  m.def("light_final_conv_bwd(Tensor g, Tensor? y, Tensor? weight, bool need_y, bool need_w, bool need_b) -> (Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("light_final_conv", &light_final_conv_cuda);
  m.impl("light_final_conv_bwd", &light_final_conv_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("light_final_conv", &light_final_conv_meta);
  m.impl("light_final_conv_bwd", &light_final_conv_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("light_final_conv", &light_final_conv_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"light_final_conv", "light_final_conv_bwd"}); }

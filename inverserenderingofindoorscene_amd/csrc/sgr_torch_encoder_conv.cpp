// torch.ops.sgrender.encoder_conv / encoder_conv_bwd: the encoders' down-sampling layers, Conv2d(C -> O, k = 4, stride = 2) behind
// ReplicationPad2d(1) or ZeroPad2d(1) (encoder0.conv1 / conv2, encoderLight.preProcess[1] / [5] / conv1 of models.py:93-115, 122-126,
// 213-246, 254-266), as operators of the C++ torch extension.
//
// Same rules as sgr_torch_light_final_conv.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_encoder_conv_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes and
// nothing synchronises.  x travels with its strides: a channels-last map or a slice is not copied.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

constexpr int64_t kMaxC = 160, kMinO = 16, kMaxO = 128;      // kEcMaxC, kEcMinO, kEcMaxO of csrc/sgr_encoder_conv.h
constexpr const char* kCompose = "; compose F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead";

struct Conv { int64_t B = 0, C = 0, O = 0, H = 0, W = 0; };

void check_sizes(const Conv& s, int64_t pad_mode, const char* who) {
  TORCH_CHECK(pad_mode == 0 || pad_mode == 1, "sgrender: ", who, ": pad_mode ", pad_mode, ", 0 (replicate) or 1 (zeros) is supported", kCompose);
  TORCH_CHECK(s.B > 0 && s.H > 0 && s.W > 0, "sgrender: ", who, ": zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.C >= 1 && s.C <= kMaxC, "sgrender: ", who, ": ", s.C, " input channels, 1..", kMaxC,
              " are supported (the deeper encoder layers are plain GEMMs with small zero-padded copies)", kCompose);
  TORCH_CHECK(s.O >= kMinO && s.O <= kMaxO && s.O % 16 == 0, "sgrender: ", who, ": ", s.O, " output channels, a multiple of 16 in ", kMinO, "..", kMaxO,
              " is supported", kCompose);
  TORCH_CHECK(s.H >= 2 && s.W >= 2, "sgrender: ", who, ": a ", s.H, " x ", s.W, " map, H and W must be at least 2", kCompose);
  TORCH_CHECK(s.B <= 65535 && (s.H / 2) * (s.W / 2) < (int64_t(1) << 26), "sgrender: ", who, ": size out of range", kCompose);
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Conv check_fwd(const Tensor& x, const Tensor& weight, const Tensor& bias, int64_t pad_mode, bool device) {
  if (device) TORCH_CHECK(x.is_cuda() && weight.is_cuda() && bias.is_cuda(), kNoCpu);
  TORCH_CHECK(x.scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat,
              "sgrender: encoder_conv: fp32 tensors required (x ", x.scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(), ")", kCompose);
  TORCH_CHECK(x.dim() == 4, "sgrender: encoder_conv: x must be [B,C,H,W], got ", x.sizes(), kCompose);
  Conv s;
  s.B = x.size(0); s.C = x.size(1); s.H = x.size(2); s.W = x.size(3);
  TORCH_CHECK(weight.dim() == 4 && weight.size(1) == s.C && weight.size(2) == 4 && weight.size(3) == 4, "sgrender: encoder_conv: weight must be [O,", s.C,
              ",4,4] (a 4x4 kernel over x's channels), got ", weight.sizes(), kCompose);
  s.O = weight.size(0);
  check_sizes(s, pad_mode, "encoder_conv");
  TORCH_CHECK(bias.dim() == 1 && bias.size(0) == s.O, "sgrender: encoder_conv: bias must be [", s.O, "], got ", bias.sizes(), kCompose);
  TORCH_CHECK(weight.device() == x.device() && bias.device() == x.device(), "sgrender: encoder_conv: tensors on different devices");
  return s;
}

Tensor encoder_conv_cuda(const Tensor& x, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const Conv s = check_fwd(x, weight, bias, pad_mode, true);
  const c10::DeviceGuard guard(x.device());
  Tensor out = at::empty({s.B, s.O, s.H / 2, s.W / 2}, x.options().memory_format(at::MemoryFormat::Contiguous));
  const Tensor w = weight.contiguous(), b = bias.contiguous();
  const Strides4 xs = strides_of(x);
  ok(api().sgr_encoder_conv_fwd(rp(x), rp(w), rp(b), wp(out), (int)s.B, (int)s.C, (int)s.O, (int)s.H, (int)s.W, xs.v, (int)pad_mode, stream_of(x.device())),
     "sgr_encoder_conv_fwd");
  return out;
}
Tensor encoder_conv_meta(const Tensor& x, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const Conv s = check_fwd(x, weight, bias, pad_mode, false);
  return at::empty({s.B, s.O, s.H / 2, s.W / 2}, x.options().memory_format(at::MemoryFormat::Contiguous));
}

// the backward's own checks.  x is needed for dweight, weight for dx; H and W are x's (the cotangent's size does not tell an odd map from an
// even one), C comes from whichever of the two tensors is there
Conv check_bwd(const Tensor& g, const OT& x, const OT& weight, int64_t H, int64_t W, int64_t pad_mode, bool nX, bool nW, bool nB, bool device) {
  TORCH_CHECK(nX || nW || nB, "sgrender: encoder_conv_bwd: no gradient requested");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == at::kFloat, "sgrender: encoder_conv_bwd: the cotangent must be fp32 [B,O,H/2,W/2], got ", g.scalar_type(), " ", g.sizes());
  Conv s;
  s.B = g.size(0); s.O = g.size(1); s.H = H; s.W = W;
  TORCH_CHECK(H >= 2 && W >= 2 && g.size(2) == H / 2 && g.size(3) == W / 2, "sgrender: encoder_conv_bwd: the cotangent must be fp32 [B,O,H/2,W/2] for H = ", H, ", W = ", W,
              ", got ", g.sizes());
  TORCH_CHECK(!nX || has(weight), "sgrender: encoder_conv_bwd: weight is needed for dx");
  TORCH_CHECK(!nW || has(x), "sgrender: encoder_conv_bwd: x is needed for dweight");
  s.C = has(weight) ? (weight->dim() == 4 ? weight->size(1) : 0) : has(x) ? (x->dim() == 4 ? x->size(1) : 0) : 1;      // dbias alone: C is not used
  if (nX) {
    if (device) TORCH_CHECK(weight->is_cuda(), kNoCpu);
    TORCH_CHECK(weight->scalar_type() == at::kFloat && weight->sizes() == at::IntArrayRef({s.O, s.C, 4, 4}), "sgrender: encoder_conv_bwd: weight must be fp32 [", s.O,
                ",C,4,4], got ", weight->scalar_type(), " ", weight->sizes());
  }
  if (nW) {
    if (device) TORCH_CHECK(x->is_cuda(), kNoCpu);
    TORCH_CHECK(x->scalar_type() == at::kFloat && x->sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: encoder_conv_bwd: x must be fp32 [", s.B, ",", s.C, ",",
                s.H, ",", s.W, "], got ", x->scalar_type(), " ", x->sizes());
  }
  check_sizes(s, pad_mode, "encoder_conv_bwd");
  return s;
}
// a [0] tensor where a gradient is not wanted
T3 bwd_outputs(const Conv& s, const at::TensorOptions& o, bool nX, bool nW, bool nB) {
  return {nX ? at::empty({s.B, s.C, s.H, s.W}, o) : none(o), nW ? at::empty({s.O, s.C, 4, 4}, o) : none(o), nB ? at::empty({s.O}, o) : none(o)};
}
T3 encoder_conv_bwd_cuda(const Tensor& g, const OT& x, const OT& weight, int64_t H, int64_t W, int64_t pad_mode, bool nX, bool nW, bool nB) {
  const Conv s = check_bwd(g, x, weight, H, W, pad_mode, nX, nW, nB, true);
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  T3 out = bwd_outputs(s, o, nX, nW, nB);
  const Tensor gc = g.contiguous();
  Tensor w, ws;
  Strides4 xs{};
  if (nX) w = weight->contiguous();
  if (nW) xs = strides_of(*x);
  if (nW || nB) {
    ws = workspace_floats(api().sgr_encoder_conv_workspace_floats((int)s.B, (int)s.C, (int)s.O, (int)s.H, (int)s.W), "encoder_conv_bwd", o);
  }
  ok(api().sgr_encoder_conv_bwd(rp(gc), nW ? rp(*x) : nullptr, rp(w), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), wp(ws), (int)s.B, (int)s.C,
                                (int)s.O, (int)s.H, (int)s.W, nW ? xs.v : nullptr, (int)pad_mode, stream_of(g.device())),
     "sgr_encoder_conv_bwd");
  return out;
}
T3 encoder_conv_bwd_meta(const Tensor& g, const OT& x, const OT& weight, int64_t H, int64_t W, int64_t pad_mode, bool nX, bool nW, bool nB) {
  const Conv s = check_bwd(g, x, weight, H, W, pad_mode, nX, nW, nB, false);
  return bwd_outputs(s, g.options().memory_format(at::MemoryFormat::Contiguous), nX, nW, nB);
}

using FwdSig = Tensor(const Tensor&, const Tensor&, const Tensor&, int64_t);
using BwdSig = T3(const Tensor&, const OT&, const OT&, int64_t, int64_t, int64_t, bool, bool, bool);

struct EncoderConvFn : public torch::autograd::Function<EncoderConvFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& weight, const Tensor& bias, int64_t pad_mode, bool nX, bool nW, bool nB) {
    Tensor out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::encoder_conv");
      out = op.call(x, weight, bias, pad_mode);
    }
    // x is kept only for dweight, the weight only for dx
    ctx->save_for_backward({nW ? x : Tensor(), nX ? weight : Tensor()});
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB;
    ctx->saved_data["H"] = x.size(2); ctx->saved_data["W"] = x.size(3); ctx->saved_data["pad_mode"] = pad_mode;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(7);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const bool nX = ctx->saved_data["nX"].toBool(), nW = ctx->saved_data["nW"].toBool(), nB = ctx->saved_data["nB"].toBool();
    static auto bwd = find_op<BwdSig>("sgrender::encoder_conv_bwd");
    auto [dx, dw, db] = bwd.call(g[0], opt_of(s[0]), opt_of(s[1]), ctx->saved_data["H"].toInt(), ctx->saved_data["W"].toInt(), ctx->saved_data["pad_mode"].toInt(), nX, nW, nB);
    if (nX) out[0] = dx;
    if (nW) out[1] = dw;
    if (nB) out[2] = db;
    return out;
  }
};

Tensor encoder_conv_autograd(const Tensor& x, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const bool grad = at::GradMode::is_enabled();
  const bool nX = grad && x.requires_grad(), nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad();
  if (!(nX || nW || nB)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::encoder_conv");
    return op.call(x, weight, bias, pad_mode);
  }
  return EncoderConvFn::apply(x, weight, bias, pad_mode, nX, nW, nB);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("encoder_conv(Tensor x, Tensor weight, Tensor bias, int pad_mode) -> Tensor");
  m.def("encoder_conv_bwd(Tensor g, Tensor? x, Tensor? weight, int H, int W, int pad_mode, bool need_x, bool need_w, bool need_b) -> (Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("encoder_conv", &encoder_conv_cuda);
  m.impl("encoder_conv_bwd", &encoder_conv_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("encoder_conv", &encoder_conv_meta);
  m.impl("encoder_conv_bwd", &encoder_conv_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("encoder_conv", &encoder_conv_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"encoder_conv", "encoder_conv_bwd"}); }

// torch.ops.sgrender.encoder_conv / encoder_conv_bwd and encoder_conv_cat / encoder_conv_cat_bwd: the encoders' down-sampling layers, Conv2d(C -> O, k = 4, stride = 2) behind
// ReplicationPad2d(1) or ZeroPad2d(1) (encoder0.conv1 / conv2, encoderLight.preProcess[1] / [5] / conv1 of models.py:93-115, 122-126,
// 213-246, 254-266), as operators of the C++ torch extension.
//
// Same rules as sgr_torch_light_final_conv.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_encoder_conv_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes and
// nothing synchronises.  x travels with its strides: a channels-last map or a slice is not copied.  The _cat operators take the layer's
// input as a list of sources (encoderLight.conv1's torch.cat([input1, input2], dim=1), models.py:254-262) and never form the concatenation.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

constexpr int64_t kMaxC = 160, kMinO = 16, kMaxO = 128;      // kEcMaxC, kEcMinO, kEcMaxO of csrc/sgr_encoder_conv.h
constexpr const char* kCompose = "; compose F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead";

struct Conv { int64_t B = 0, C = 0, O = 0, H = 0, W = 0; };

// compose: the composition a refusal names
void check_sizes(const Conv& s, int64_t pad_mode, const char* who, const char* compose = kCompose) {
  TORCH_CHECK(pad_mode == 0 || pad_mode == 1, "sgrender: ", who, ": pad_mode ", pad_mode, ", 0 (replicate) or 1 (zeros) is supported", compose);
  TORCH_CHECK(s.B > 0 && s.H > 0 && s.W > 0, "sgrender: ", who, ": zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.C >= 1 && s.C <= kMaxC, "sgrender: ", who, ": ", s.C, " input channels, 1..", kMaxC,
              " are supported (the deeper encoder layers are plain GEMMs with small zero-padded copies)", compose);
  TORCH_CHECK(s.O >= kMinO && s.O <= kMaxO && s.O % 16 == 0, "sgrender: ", who, ": ", s.O, " output channels, a multiple of 16 in ", kMinO, "..", kMaxO,
              " is supported", compose);
  TORCH_CHECK(s.H >= 2 && s.W >= 2, "sgrender: ", who, ": a ", s.H, " x ", s.W, " map, H and W must be at least 2", compose);
  TORCH_CHECK(s.B <= 65535 && (s.H / 2) * (s.W / 2) < (int64_t(1) << 26), "sgrender: ", who, ": size out of range", compose);
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


// ---- several sources: encoder_conv_cat / encoder_conv_cat_bwd -----------------------------------------------------------------------------------
// The convolution of torch.cat(xs, 1), bit for bit, without the concatenated copy.  The sources' pointers, channel counts and strides travel
// as host arrays into the kernel arguments: no device-side table.  Where a list entry is absent (a source the backward does not read, a
// gradient nobody wants) it is a [0] tensor.
using TL = at::TensorList;
using TV = std::vector<Tensor>;
using CatBwdOut = std::tuple<TV, Tensor, Tensor>;

constexpr int64_t kMaxSources = SGR_ENCODER_CONV_MAX_SOURCES;
constexpr const char* kComposeCat = "; compose torch.cat(xs, 1), F.pad(x, (1, 1, 1, 1), mode=...) and F.conv2d(., stride=2) instead";

struct Cat {
  Conv s;
  std::vector<int64_t> channels;
};

void check_count(int64_t S, const char* who) {
  TORCH_CHECK(S >= 1 && S <= kMaxSources, "sgrender: ", who, ": the number of sources must be 1 .. ", kMaxSources, ", got ", S, kComposeCat);
}
void check_cat_sizes(const Cat& c, int64_t pad_mode, const char* who) {
  for (const int64_t ci : c.channels)
    TORCH_CHECK(ci >= 1, "sgrender: ", who, ": a source with ", ci, " channels, every source needs at least one", kComposeCat);
  TORCH_CHECK(c.s.C <= kMaxC, "sgrender: ", who, ": ", c.s.C, " input channels, 1..", kMaxC,
              " are supported (the deeper encoder layers are plain GEMMs with small zero-padded copies)", kComposeCat);
  check_sizes(c.s, pad_mode, who, kComposeCat);
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Cat check_cat_fwd(TL xs, const Tensor& weight, const Tensor& bias, int64_t pad_mode, bool device) {
  const char* who = "encoder_conv_cat";
  check_count((int64_t)xs.size(), who);
  const Tensor& x0 = xs[0];
  Cat c;
  for (size_t i = 0; i < xs.size(); ++i) {
    if (device) TORCH_CHECK(xs[i].is_cuda() && weight.is_cuda() && bias.is_cuda(), kNoCpu);
    TORCH_CHECK(xs[i].scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat,
                "sgrender: encoder_conv_cat: fp32 tensors required (xs[", i, "] ", xs[i].scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(), ")",
                kComposeCat);
    TORCH_CHECK(xs[i].dim() == 4, "sgrender: encoder_conv_cat: xs[", i, "] must be [B,C,H,W], got ", xs[i].sizes(), kComposeCat);
    TORCH_CHECK(xs[i].size(0) == x0.size(0) && xs[i].size(2) == x0.size(2) && xs[i].size(3) == x0.size(3),
                "sgrender: encoder_conv_cat: the sources must have one batch and one plane, got xs[0] ", x0.sizes(), " and xs[", i, "] ", xs[i].sizes(), kComposeCat);
    TORCH_CHECK(xs[i].device() == x0.device(), "sgrender: encoder_conv_cat: tensors on different devices");
    c.channels.push_back(xs[i].size(1));
    c.s.C += xs[i].size(1);
  }
  c.s.B = x0.size(0); c.s.H = x0.size(2); c.s.W = x0.size(3);
  TORCH_CHECK(weight.dim() == 4 && weight.size(1) == c.s.C && weight.size(2) == 4 && weight.size(3) == 4, "sgrender: encoder_conv_cat: weight must be [O,", c.s.C,
              ",4,4] (a 4x4 kernel over the summed channels of xs), got ", weight.sizes(), kComposeCat);
  c.s.O = weight.size(0);
  check_cat_sizes(c, pad_mode, who);
  TORCH_CHECK(bias.dim() == 1 && bias.size(0) == c.s.O, "sgrender: encoder_conv_cat: bias must be [", c.s.O, "], got ", bias.sizes(), kComposeCat);
  TORCH_CHECK(weight.device() == x0.device() && bias.device() == x0.device(), "sgrender: encoder_conv_cat: tensors on different devices");
  return c;
}

// S device pointers, channel counts and S x 4 strides for the C ABI, which reads them during the call
struct Table {
  const float* p[SGR_ENCODER_CONV_MAX_SOURCES] = {};
  int channels[SGR_ENCODER_CONV_MAX_SOURCES] = {};
  long long strides[4 * SGR_ENCODER_CONV_MAX_SOURCES] = {};
};
Table table_of(TL xs, const std::vector<int64_t>& channels) {
  Table t;
  for (size_t i = 0; i < channels.size(); ++i) {
    t.channels[i] = (int)channels[i];
    if (i < xs.size() && present(xs[i])) {
      t.p[i] = rp(xs[i]);
      for (int k = 0; k < 4; ++k) t.strides[4 * i + k] = (long long)xs[i].stride(k);
    }
  }
  return t;
}

Tensor encoder_conv_cat_cuda(TL xs, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const Cat c = check_cat_fwd(xs, weight, bias, pad_mode, true);
  const Conv& s = c.s;
  const c10::DeviceGuard guard(xs[0].device());
  Tensor out = at::empty({s.B, s.O, s.H / 2, s.W / 2}, xs[0].options().memory_format(at::MemoryFormat::Contiguous));
  const Tensor w = weight.contiguous(), b = bias.contiguous();
  const Table t = table_of(xs, c.channels);
  ok(api().sgr_encoder_conv_cat_fwd((int)xs.size(), t.p, t.channels, t.strides, rp(w), rp(b), wp(out), (int)s.B, (int)s.O, (int)s.H, (int)s.W, (int)pad_mode,
                                    stream_of(xs[0].device())),
     "sgr_encoder_conv_cat_fwd");
  return out;
}
Tensor encoder_conv_cat_meta(TL xs, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const Cat c = check_cat_fwd(xs, weight, bias, pad_mode, false);
  return at::empty({c.s.B, c.s.O, c.s.H / 2, c.s.W / 2}, xs[0].options().memory_format(at::MemoryFormat::Contiguous));
}

// the backward's own checks.  channels: the sources' channel counts, always given (they place a source's channels in the weight).  nX: bit i
// set = dxs[i] is wanted.  xs are needed for dweight alone and may be [0] tensors otherwise; the weight is needed for any dx
Cat check_cat_bwd(const Tensor& g, TL xs, const OT& weight, at::IntArrayRef channels, int64_t H, int64_t W, int64_t pad_mode, int64_t nX, bool nW, bool nB, bool device) {
  const char* who = "encoder_conv_cat_bwd";
  const int64_t S = (int64_t)channels.size();
  check_count(S, who);
  TORCH_CHECK((int64_t)xs.size() == S, "sgrender: encoder_conv_cat_bwd: ", S, " channel counts but ", xs.size(), " xs");
  TORCH_CHECK((nX & ~((int64_t(1) << S) - 1)) == 0, "sgrender: encoder_conv_cat_bwd: a gradient requested for a source that does not exist");
  TORCH_CHECK(nX || nW || nB, "sgrender: encoder_conv_cat_bwd: no gradient requested");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == at::kFloat, "sgrender: encoder_conv_cat_bwd: the cotangent must be fp32 [B,O,H/2,W/2], got ", g.scalar_type(), " ", g.sizes());
  Cat c;
  c.channels = channels.vec();
  for (const int64_t ci : channels) c.s.C += ci;
  c.s.B = g.size(0); c.s.O = g.size(1); c.s.H = H; c.s.W = W;
  TORCH_CHECK(H >= 2 && W >= 2 && g.size(2) == H / 2 && g.size(3) == W / 2, "sgrender: encoder_conv_cat_bwd: the cotangent must be fp32 [B,O,H/2,W/2] for H = ", H,
              ", W = ", W, ", got ", g.sizes());
  TORCH_CHECK(!nX || has(weight), "sgrender: encoder_conv_cat_bwd: weight is needed for dx");
  if (nX) {
    if (device) TORCH_CHECK(weight->is_cuda(), kNoCpu);
    TORCH_CHECK(weight->scalar_type() == at::kFloat && weight->sizes() == at::IntArrayRef({c.s.O, c.s.C, 4, 4}), "sgrender: encoder_conv_cat_bwd: weight must be fp32 [", c.s.O,
                ",", c.s.C, ",4,4], got ", weight->scalar_type(), " ", weight->sizes());
  }
  for (int64_t i = 0; nW && i < S; ++i) {
    TORCH_CHECK(present(xs[i]), "sgrender: encoder_conv_cat_bwd: xs are needed for dweight");
    if (device) TORCH_CHECK(xs[i].is_cuda(), kNoCpu);
    TORCH_CHECK(xs[i].scalar_type() == at::kFloat && xs[i].sizes() == at::IntArrayRef({c.s.B, channels[i], H, W}), "sgrender: encoder_conv_cat_bwd: xs[", i, "] must be fp32 [",
                c.s.B, ",", channels[i], ",", H, ",", W, "], got ", xs[i].scalar_type(), " ", xs[i].sizes());
  }
  check_cat_sizes(c, pad_mode, who);
  return c;
}
// a [0] tensor where a gradient is not wanted
CatBwdOut cat_bwd_outputs(const Cat& c, const at::TensorOptions& o, int64_t nX, bool nW, bool nB) {
  TV dxs;
  for (size_t i = 0; i < c.channels.size(); ++i) dxs.push_back(((nX >> i) & 1) ? at::empty({c.s.B, c.channels[i], c.s.H, c.s.W}, o) : none(o));
  return {dxs, nW ? at::empty({c.s.O, c.s.C, 4, 4}, o) : none(o), nB ? at::empty({c.s.O}, o) : none(o)};
}
CatBwdOut encoder_conv_cat_bwd_cuda(const Tensor& g, TL xs, const OT& weight, at::IntArrayRef channels, int64_t H, int64_t W, int64_t pad_mode, int64_t nX, bool nW,
                                    bool nB) {
  const Cat c = check_cat_bwd(g, xs, weight, channels, H, W, pad_mode, nX, nW, nB, true);
  const Conv& s = c.s;
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  CatBwdOut out = cat_bwd_outputs(c, o, nX, nW, nB);
  const Tensor gc = g.contiguous();
  Tensor w, ws;
  if (nX) w = weight->contiguous();
  if (nW || nB) ws = workspace_floats(api().sgr_encoder_conv_workspace_floats((int)s.B, (int)s.C, (int)s.O, (int)s.H, (int)s.W), "encoder_conv_cat_bwd", o);
  const Table t = nW ? table_of(xs, c.channels) : table_of({}, c.channels);
  float* dxs[SGR_ENCODER_CONV_MAX_SOURCES] = {};
  for (size_t i = 0; i < c.channels.size(); ++i) dxs[i] = wp(std::get<0>(out)[i]);
  ok(api().sgr_encoder_conv_cat_bwd((int)c.channels.size(), rp(gc), nW ? t.p : nullptr, t.channels, nW ? t.strides : nullptr, rp(w), dxs, wp(std::get<1>(out)),
                                    wp(std::get<2>(out)), wp(ws), (int)s.B, (int)s.O, (int)s.H, (int)s.W, (int)pad_mode, stream_of(g.device())),
     "sgr_encoder_conv_cat_bwd");
  return out;
}
CatBwdOut encoder_conv_cat_bwd_meta(const Tensor& g, TL xs, const OT& weight, at::IntArrayRef channels, int64_t H, int64_t W, int64_t pad_mode, int64_t nX, bool nW,
                                    bool nB) {
  const Cat c = check_cat_bwd(g, xs, weight, channels, H, W, pad_mode, nX, nW, nB, false);
  return cat_bwd_outputs(c, g.options().memory_format(at::MemoryFormat::Contiguous), nX, nW, nB);
}

using CatFwdSig = Tensor(TL, const Tensor&, const Tensor&, int64_t);
using CatBwdSig = CatBwdOut(const Tensor&, TL, const OT&, at::IntArrayRef, int64_t, int64_t, int64_t, int64_t, bool, bool);

struct EncoderConvCatFn : public torch::autograd::Function<EncoderConvCatFn> {
  static Tensor forward(AutogradContext* ctx, TL xs, const Tensor& weight, const Tensor& bias, int64_t pad_mode, int64_t nX, bool nW, bool nB) {
    Tensor out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<CatFwdSig>("sgrender::encoder_conv_cat");
      out = op.call(xs, weight, bias, pad_mode);
    }
    // the sources are kept only for dweight, the weight only for some dx
    variable_list keep;
    std::vector<int64_t> channels;
    for (const Tensor& x : xs) {
      keep.push_back(nW ? x : Tensor());
      channels.push_back(x.size(1));
    }
    keep.push_back(nX ? weight : Tensor());
    ctx->save_for_backward(keep);
    ctx->saved_data["channels"] = channels;
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB;
    ctx->saved_data["H"] = xs[0].size(2); ctx->saved_data["W"] = xs[0].size(3); ctx->saved_data["pad_mode"] = pad_mode;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    const std::vector<int64_t> channels = ctx->saved_data["channels"].toIntVector();
    const size_t S = channels.size();
    variable_list out(S + 6);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const int64_t nX = ctx->saved_data["nX"].toInt();
    const bool nW = ctx->saved_data["nW"].toBool(), nB = ctx->saved_data["nB"].toBool();
    TV xs;
    const Tensor absent = none_like(g[0]);
    for (size_t i = 0; i < S; ++i) xs.push_back(nW ? s[i] : absent);
    static auto bwd = find_op<CatBwdSig>("sgrender::encoder_conv_cat_bwd");
    auto [dxs, dw, db] = bwd.call(g[0], xs, opt_of(s[S]), channels, ctx->saved_data["H"].toInt(), ctx->saved_data["W"].toInt(), ctx->saved_data["pad_mode"].toInt(), nX, nW, nB);
    for (size_t i = 0; i < S; ++i)
      if ((nX >> i) & 1) out[i] = dxs[i];
    if (nW) out[S] = dw;
    if (nB) out[S + 1] = db;
    return out;
  }
};

Tensor encoder_conv_cat_autograd(TL xs, const Tensor& weight, const Tensor& bias, int64_t pad_mode) {
  const bool grad = at::GradMode::is_enabled();
  int64_t nX = 0;
  for (size_t i = 0; grad && i < xs.size() && i < (size_t)kMaxSources; ++i) nX |= int64_t(xs[i].requires_grad()) << i;
  const bool nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad();
  const bool listed = xs.size() >= 1 && xs.size() <= (size_t)kMaxSources;      // the operator below refuses any other list
  if (!listed || !(nX || nW || nB)) {      // nothing to differentiate (or a call the operator refuses): no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<CatFwdSig>("sgrender::encoder_conv_cat");
    return op.call(xs, weight, bias, pad_mode);
  }
  return EncoderConvCatFn::apply(xs, weight, bias, pad_mode, nX, nW, nB);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("encoder_conv(Tensor x, Tensor weight, Tensor bias, int pad_mode) -> Tensor");
  m.def("encoder_conv_bwd(Tensor g, Tensor? x, Tensor? weight, int H, int W, int pad_mode, bool need_x, bool need_w, bool need_b) -> (Tensor, Tensor, Tensor)");
  m.def("encoder_conv_cat(Tensor[] xs, Tensor weight, Tensor bias, int pad_mode) -> Tensor");
  m.def("encoder_conv_cat_bwd(Tensor g, Tensor[] xs, Tensor? weight, int[] channels, int H, int W, int pad_mode, int need_x, bool need_w, bool need_b) -> "
        "(Tensor[], Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("encoder_conv", &encoder_conv_cuda);
  m.impl("encoder_conv_bwd", &encoder_conv_bwd_cuda);
  m.impl("encoder_conv_cat", &encoder_conv_cat_cuda);
  m.impl("encoder_conv_cat_bwd", &encoder_conv_cat_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("encoder_conv", &encoder_conv_meta);
  m.impl("encoder_conv_bwd", &encoder_conv_bwd_meta);
  m.impl("encoder_conv_cat", &encoder_conv_cat_meta);
  m.impl("encoder_conv_cat_bwd", &encoder_conv_cat_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) {
  m.impl("encoder_conv", &encoder_conv_autograd);
  m.impl("encoder_conv_cat", &encoder_conv_cat_autograd);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"encoder_conv", "encoder_conv_bwd", "encoder_conv_cat", "encoder_conv_cat_bwd"}); }

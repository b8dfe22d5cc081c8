// torch.ops.sgrender.gn_resize / gn_resize_bwd: the decoder stage of sgr_torch_gn_stage.cpp with the reference's resize-to-skip branch
// taken (models.py:165-166, 170-171, 175-176, 180-181, 185-186; decoderLight: 312-313 ... 332-333): GroupNorm + ReLU, a bilinear resize to
// [out_h, out_w], then -- with a skip of that size -- the concatenation and the 2x bilinear upsample.
//
// Same rules as sgr_torch_gn_stage.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_gn_resize_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes and
// nothing synchronises.  x and skip travel with their strides.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

struct Resize {
  int64_t B = 0, C = 0, Cs = 0, H = 0, W = 0, Hs = 0, Ws = 0, G = 0;
  bool up() const { return Cs > 0; }
  std::vector<int64_t> out_sizes() const { return up() ? std::vector<int64_t>{B, C + Cs, 2 * Hs, 2 * Ws} : std::vector<int64_t>{B, C, Hs, Ws}; }
};

constexpr const char* kOutside =
    "the fused resize covers H <= h <= 2H and W <= w <= 2W per axis (what floor-halving encoders and doubling decoders produce); any other "
    "size stays the caller's -- group_norm_relu(x, ...), then F.interpolate(., [h, w], mode='bilinear'), torch.cat and "
    "F.interpolate(., scale_factor=2, mode='bilinear')";

// sizes alone: shared by the forward and the backward, the device and the Meta kernels
void check_sizes(const Resize& s, const char* who) {
  TORCH_CHECK(s.B > 0 && s.C > 0 && s.H > 0 && s.W > 0, "sgrender: ", who, ": zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.G > 0 && s.C % s.G == 0, "sgrender: ", who, ": the channel count ", s.C, " is not a multiple of num_groups ", s.G);
  TORCH_CHECK(s.Hs > 0 && s.Ws > 0, "sgrender: ", who, ": the target size must be positive, got ", s.Hs, "x", s.Ws);
  TORCH_CHECK(s.Hs >= s.H && s.Hs <= 2 * s.H && s.Ws >= s.W && s.Ws <= 2 * s.W, "sgrender: ", who, ": the target ", s.Hs, "x", s.Ws, " is outside the resize domain of x ", s.H,
              "x", s.W, "; ", kOutside);
  TORCH_CHECK(s.B <= 65535 && s.C + s.Cs <= 65535 && s.Hs * s.Ws < (int64_t(1) << 26), "sgrender: ", who, ": size out of range");
}

Resize check_fwd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, int64_t out_h, int64_t out_w, double eps, bool device) {
  if (device) TORCH_CHECK(x.is_cuda() && weight.is_cuda() && bias.is_cuda() && (!has(skip) || skip->is_cuda()), kNoCpu);
  TORCH_CHECK(x.scalar_type() == at::kFloat && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat &&
                  (!has(skip) || skip->scalar_type() == at::kFloat),
              "sgrender: gn_resize: fp32 tensors required (x ", x.scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(),
              has(skip) ? ", skip " : "", has(skip) ? c10::toString(skip->scalar_type()) : "", ")");
  TORCH_CHECK(x.dim() == 4, "sgrender: gn_resize: x must be [B,C,H,W], got ", x.sizes());
  Resize s;
  s.B = x.size(0); s.C = x.size(1); s.H = x.size(2); s.W = x.size(3); s.G = G; s.Hs = out_h; s.Ws = out_w;
  if (has(skip)) {
    TORCH_CHECK(skip->dim() == 4 && skip->size(0) == s.B && skip->size(1) >= 1 && skip->size(2) == out_h && skip->size(3) == out_w, "sgrender: gn_resize: skip must be [", s.B,
                ",Cs,", out_h, ",", out_w, "] with Cs >= 1, got ", skip->sizes());
    TORCH_CHECK(skip->device() == x.device(), "sgrender: gn_resize: tensors on different devices");
    s.Cs = skip->size(1);
  }
  check_sizes(s, "gn_resize");
  TORCH_CHECK(weight.dim() == 1 && weight.size(0) == s.C && bias.dim() == 1 && bias.size(0) == s.C, "sgrender: gn_resize: weight and bias must be [", s.C, "], got ",
              weight.sizes(), " and ", bias.sizes());
  TORCH_CHECK(eps > 0, "sgrender: gn_resize: eps must be positive");
  TORCH_CHECK(weight.device() == x.device() && bias.device() == x.device(), "sgrender: gn_resize: tensors on different devices");
  return s;
}

Tensor workspace(const Resize& s, bool backward, const at::TensorOptions& o) {
  return workspace_floats(api().sgr_gn_resize_workspace_floats((int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, (int)s.Hs, (int)s.Ws, s.up(), backward), "gn_resize", o);
}

// -> (out, stats [B,G,4])
T2 gn_resize_cuda(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, int64_t out_h, int64_t out_w, double eps) {
  const Resize s = check_fwd(x, weight, bias, skip, G, out_h, out_w, eps, true);
  const c10::DeviceGuard guard(x.device());
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous);
  Tensor out = at::empty(s.out_sizes(), o), stats = at::empty({s.B, s.G, 4}, o);
  const Tensor w = weight.contiguous(), b = bias.contiguous(), ws = workspace(s, false, o);
  const Strides4 xs = strides_of(x), ss = has(skip) ? strides_of(*skip) : Strides4{};
  ok(api().sgr_gn_resize_fwd(rp(x), rp(w), rp(b), has(skip) ? rp(*skip) : nullptr, wp(out), wp(stats), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H,
                             (int)s.W, (int)s.Hs, (int)s.Ws, xs.v, has(skip) ? ss.v : nullptr, (float)eps, stream_of(x.device())),
     "sgr_gn_resize_fwd");
  return {out, stats};
}
T2 gn_resize_meta(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, int64_t out_h, int64_t out_w, double eps) {
  const Resize s = check_fwd(x, weight, bias, skip, G, out_h, out_w, eps, false);
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous);
  return {at::empty(s.out_sizes(), o), at::empty({s.B, s.G, 4}, o)};
}

// the backward's own checks; x / weight / bias / stats may be None when only dskip is wanted.  H, W: the sizes of x.
Resize check_bwd(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, bool nX, bool nW,
                 bool nB, bool nS, bool device) {
  TORCH_CHECK(nX || nW || nB || nS, "sgrender: gn_resize_bwd: no gradient requested");
  TORCH_CHECK(!nS || Cs > 0, "sgrender: gn_resize_bwd: a skip gradient requested without skip channels");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && g.scalar_type() == at::kFloat && C > 0 && Cs >= 0 && g.size(1) == C + Cs, "sgrender: gn_resize_bwd: the cotangent must be fp32 [B,", C + Cs,
              ",.,.], got ", g.scalar_type(), " ", g.sizes());
  Resize s;
  s.B = g.size(0); s.C = C; s.Cs = Cs; s.G = G; s.H = H; s.W = W;
  s.Hs = Cs > 0 ? g.size(2) / 2 : g.size(2);
  s.Ws = Cs > 0 ? g.size(3) / 2 : g.size(3);
  TORCH_CHECK(g.sizes() == at::IntArrayRef(s.out_sizes()), "sgrender: gn_resize_bwd: the cotangent of an upsampled result must have even sizes, got ", g.sizes());
  check_sizes(s, "gn_resize_bwd");
  if (nX || nW || nB) {
    TORCH_CHECK(has(x) && has(weight) && has(bias) && has(stats), "sgrender: gn_resize_bwd: x, weight, bias and stats are needed for dx, dweight and dbias");
    if (device) TORCH_CHECK(x->is_cuda() && weight->is_cuda() && bias->is_cuda() && stats->is_cuda(), kNoCpu);
    TORCH_CHECK(x->scalar_type() == at::kFloat && x->sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: gn_resize_bwd: x must be fp32 [", s.B, ",", s.C, ",", s.H, ",",
                s.W, "], got ", x->scalar_type(), " ", x->sizes());
    TORCH_CHECK(weight->scalar_type() == at::kFloat && bias->scalar_type() == at::kFloat && weight->dim() == 1 && bias->dim() == 1 && weight->size(0) == s.C &&
                    bias->size(0) == s.C,
                "sgrender: gn_resize_bwd: weight and bias must be fp32 [", s.C, "]");
    TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->sizes() == at::IntArrayRef({s.B, s.G, 4}), "sgrender: gn_resize_bwd: stats must be fp32 [", s.B, ",", s.G,
                ",4], got ", stats->sizes());
  }
  return s;
}
// a [0] tensor where a gradient is not wanted
T4 bwd_outputs(const Resize& s, const at::TensorOptions& o, bool nX, bool nW, bool nB, bool nS) {
  return {nX ? at::empty({s.B, s.C, s.H, s.W}, o) : none(o), nW ? at::empty({s.C}, o) : none(o), nB ? at::empty({s.C}, o) : none(o),
          nS ? at::empty({s.B, s.Cs, s.Hs, s.Ws}, o) : none(o)};
}
T4 gn_resize_bwd_cuda(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, bool nX,
                      bool nW, bool nB, bool nS) {
  const Resize s = check_bwd(g, x, weight, bias, stats, C, Cs, G, H, W, nX, nW, nB, nS, true);
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  const bool side = nX || nW || nB;
  T4 out = bwd_outputs(s, o, nX, nW, nB, nS);
  const Tensor gc = g.contiguous();
  Tensor w, b, st, ws;
  Strides4 xs{};
  if (side) {
    w = weight->contiguous(); b = bias->contiguous(); st = stats->contiguous();
    ws = workspace(s, true, o);
    xs = strides_of(*x);
  }
  ok(api().sgr_gn_resize_bwd(rp(gc), side ? rp(*x) : nullptr, rp(w), rp(b), rp(st), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)),
                             wp(std::get<3>(out)), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, (int)s.Hs, (int)s.Ws, side ? xs.v : nullptr,
                             stream_of(g.device())),
     "sgr_gn_resize_bwd");
  return out;
}
T4 gn_resize_bwd_meta(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, bool nX,
                      bool nW, bool nB, bool nS) {
  const Resize s = check_bwd(g, x, weight, bias, stats, C, Cs, G, H, W, nX, nW, nB, nS, false);
  return bwd_outputs(s, g.options().memory_format(at::MemoryFormat::Contiguous), nX, nW, nB, nS);
}

using FwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const OT&, int64_t, int64_t, int64_t, double);
using BwdSig = T4(const Tensor&, const OT&, const OT&, const OT&, const OT&, int64_t, int64_t, int64_t, int64_t, int64_t, bool, bool, bool, bool);

struct GnResizeFn : public torch::autograd::Function<GnResizeFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, int64_t out_h, int64_t out_w,
                               double eps, bool nX, bool nW, bool nB, bool nS) {
    T2 out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::gn_resize");
      out = op.call(x, weight, bias, skip, G, out_h, out_w, eps);
    }
    // what gn_stage's node keeps and the sizes: no resized map, no concatenated map, no skip (its gradient is linear in the cotangent)
    const bool side = nX || nW || nB;
    ctx->save_for_backward({side ? x : Tensor(), side ? weight : Tensor(), side ? bias : Tensor(), side ? std::get<1>(out) : Tensor()});
    ctx->saved_data["C"] = x.size(1);
    ctx->saved_data["Cs"] = has(skip) ? skip->size(1) : (int64_t)0;
    ctx->saved_data["G"] = G;
    ctx->saved_data["H"] = x.size(2);
    ctx->saved_data["W"] = x.size(3);
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB; ctx->saved_data["nS"] = nS;
    ctx->mark_non_differentiable({std::get<1>(out)});
    return {std::get<0>(out), std::get<1>(out)};
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(12);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const bool need[4] = {ctx->saved_data["nX"].toBool(), ctx->saved_data["nW"].toBool(), ctx->saved_data["nB"].toBool(), ctx->saved_data["nS"].toBool()};
    static auto bwd = find_op<BwdSig>("sgrender::gn_resize_bwd");
    auto [dx, dw, db, ds] = bwd.call(g[0], opt_of(s[0]), opt_of(s[1]), opt_of(s[2]), opt_of(s[3]), ctx->saved_data["C"].toInt(), ctx->saved_data["Cs"].toInt(),
                                     ctx->saved_data["G"].toInt(), ctx->saved_data["H"].toInt(), ctx->saved_data["W"].toInt(), need[0], need[1], need[2], need[3]);
    if (need[0]) out[0] = dx;
    if (need[1]) out[1] = dw;
    if (need[2]) out[2] = db;
    if (need[3]) out[3] = ds;
    return out;
  }
};

T2 gn_resize_autograd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, int64_t out_h, int64_t out_w, double eps) {
  const bool grad = at::GradMode::is_enabled();
  const bool nX = grad && x.requires_grad(), nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad(), nS = grad && has(skip) && skip->requires_grad();
  if (!(nX || nW || nB || nS)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::gn_resize");
    return op.call(x, weight, bias, skip, G, out_h, out_w, eps);
  }
  auto o = GnResizeFn::apply(x, weight, bias, skip, G, out_h, out_w, eps, nX, nW, nB, nS);
  return {o[0], o[1]};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("gn_resize(Tensor x, Tensor weight, Tensor bias, Tensor? skip, int num_groups, int out_h, int out_w, float eps=1e-05) -> (Tensor, Tensor)");
  m.def("gn_resize_bwd(Tensor g, Tensor? x, Tensor? weight, Tensor? bias, Tensor? stats, int channels, int skip_channels, int num_groups, int height, int width, "
        "bool need_x, bool need_weight, bool need_bias, bool need_skip) -> (Tensor, Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("gn_resize", &gn_resize_cuda);
  m.impl("gn_resize_bwd", &gn_resize_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("gn_resize", &gn_resize_meta);
  m.impl("gn_resize_bwd", &gn_resize_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("gn_resize", &gn_resize_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"gn_resize", "gn_resize_bwd"}); }

// torch.ops.sgrender.gn_stage / gn_stage_bwd: GroupNorm + ReLU, optionally followed by the skip concatenation and the 2x bilinear upsample
// (the repeated stage of models.encoder0 / decoder0 / encoderLight / decoderLight, models.py:122-127, 160-183), as operators of the C++
// torch extension.
//
// Same rules as sgr_torch_brdf_heads.cpp: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_gn_stage_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes and nothing
// synchronises.  x and skip travel with their strides: a channels-last convolution output is not copied.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

// the element types of x, skip, the result, the cotangent, dx and dskip; everything else is fp32
bool io_type(at::ScalarType t) { return t == at::kFloat || t == at::kBFloat16; }
// a bf16 tensor's elements as the C ABI takes them; absent and empty tensors are NULL
const unsigned short* hrp(const Tensor& t) { return t.defined() && t.numel() ? static_cast<const unsigned short*>(t.const_data_ptr()) : nullptr; }
unsigned short* hwp(const Tensor& t) { return t.defined() && t.numel() ? static_cast<unsigned short*>(t.mutable_data_ptr()) : nullptr; }

struct Stage {
  int64_t B = 0, C = 0, Cs = 0, H = 0, W = 0, G = 0;
  bool up() const { return Cs > 0; }
  std::vector<int64_t> out_sizes() const { return up() ? std::vector<int64_t>{B, C + Cs, 2 * H, 2 * W} : std::vector<int64_t>{B, C, H, W}; }
};

constexpr const char* kResize =
    "the reference resizes the normalised map to the skip in that case (models.py:165-166, 170-171, 175-176, 180-181; decoderLight: 312-313, "
    "317-318, 322-323, 327-328): that branch stays the caller's -- group_norm_relu(x, ...), then F.interpolate(., [h, w], mode='bilinear'), "
    "torch.cat and F.interpolate(., scale_factor=2, mode='bilinear')";

void check_sizes(const Stage& s) {
  TORCH_CHECK(s.B > 0 && s.C > 0 && s.H > 0 && s.W > 0, "sgrender: gn_stage: zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.G > 0 && s.C % s.G == 0, "sgrender: gn_stage: the channel count ", s.C, " is not a multiple of num_groups ", s.G);
  TORCH_CHECK(s.B <= 65535 && s.C + s.Cs <= 65535 && s.H * s.W < (int64_t(1) << 26), "sgrender: gn_stage: size out of range");
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Stage check_fwd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps, bool device) {
  if (device) TORCH_CHECK(x.is_cuda() && weight.is_cuda() && bias.is_cuda() && (!has(skip) || skip->is_cuda()), kNoCpu);
  // x and skip: fp32, or bf16 together; weight and bias: fp32 either way, as autocast leaves parameters
  const auto xt = x.scalar_type();
  if (has(skip) && io_type(xt) && io_type(skip->scalar_type()))
    TORCH_CHECK(skip->scalar_type() == xt, "sgrender: gn_stage: x and skip must have one dtype, got x ", xt, " and skip ", skip->scalar_type(),
                "; cast one of them (under torch.autocast the operator casts skip to x's dtype itself)");
  if (xt == at::kBFloat16)
    TORCH_CHECK(weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat, "sgrender: gn_stage: a bf16 x takes fp32 weight and bias (the parameters stay fp32, as "
                "under torch.autocast), got weight ", weight.scalar_type(), " and bias ", bias.scalar_type());
  TORCH_CHECK(io_type(xt) && weight.scalar_type() == at::kFloat && bias.scalar_type() == at::kFloat && (!has(skip) || skip->scalar_type() == xt),
              "sgrender: gn_stage: fp32 tensors required (x ", x.scalar_type(), ", weight ", weight.scalar_type(), ", bias ", bias.scalar_type(),
              has(skip) ? ", skip " : "", has(skip) ? c10::toString(skip->scalar_type()) : "", ")");
  TORCH_CHECK(x.dim() == 4, "sgrender: gn_stage: x must be [B,C,H,W], got ", x.sizes());
  Stage s;
  s.B = x.size(0); s.C = x.size(1); s.H = x.size(2); s.W = x.size(3); s.G = G;
  check_sizes(s);
  TORCH_CHECK(weight.dim() == 1 && weight.size(0) == s.C && bias.dim() == 1 && bias.size(0) == s.C, "sgrender: gn_stage: weight and bias must be [", s.C,
              "], got ", weight.sizes(), " and ", bias.sizes());
  TORCH_CHECK(eps > 0, "sgrender: gn_stage: eps must be positive");
  TORCH_CHECK(weight.device() == x.device() && bias.device() == x.device(), "sgrender: gn_stage: tensors on different devices");
  if (has(skip)) {
    TORCH_CHECK(skip->device() == x.device(), "sgrender: gn_stage: tensors on different devices");
    TORCH_CHECK(skip->dim() == 4 && skip->size(0) == s.B && skip->size(1) >= 1, "sgrender: gn_stage: skip must be [", s.B, ",Cs,", s.H, ",", s.W, "] with Cs >= 1, got ",
                skip->sizes());
    TORCH_CHECK(skip->size(2) == s.H && skip->size(3) == s.W, "sgrender: gn_stage: skip is ", skip->size(2), "x", skip->size(3), " but x is ", s.H, "x", s.W, "; ", kResize);
    s.Cs = skip->size(1);
    check_sizes(s);
  }
  return s;
}

Tensor workspace(const Stage& s, bool backward, const at::TensorOptions& o) {
  return workspace_floats(api().sgr_gn_stage_workspace_floats((int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, s.up(), backward), "gn_stage", o);
}

// -> (out, stats [B,G,4])
T2 gn_stage_cuda(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps) {
  const Stage s = check_fwd(x, weight, bias, skip, G, eps, true);
  const c10::DeviceGuard guard(x.device());
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous), of = o.dtype(at::kFloat);
  Tensor out = at::empty(s.out_sizes(), o), stats = at::empty({s.B, s.G, 4}, of);
  const Tensor w = weight.contiguous(), b = bias.contiguous(), ws = workspace(s, false, of);
  const Strides4 xs = strides_of(x), ss = has(skip) ? strides_of(*skip) : Strides4{};
  if (x.scalar_type() == at::kBFloat16) {
    ok(api().sgr_gn_stage_fwd_bf16(hrp(x), rp(w), rp(b), has(skip) ? hrp(*skip) : nullptr, hwp(out), wp(stats), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs,
                                   (int)s.H, (int)s.W, xs.v, has(skip) ? ss.v : nullptr, (float)eps, stream_of(x.device())),
       "sgr_gn_stage_fwd_bf16");
    return {out, stats};
  }
  ok(api().sgr_gn_stage_fwd(rp(x), rp(w), rp(b), has(skip) ? rp(*skip) : nullptr, wp(out), wp(stats), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H,
                            (int)s.W, xs.v, has(skip) ? ss.v : nullptr, (float)eps, stream_of(x.device())),
     "sgr_gn_stage_fwd");
  return {out, stats};
}
T2 gn_stage_meta(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps) {
  const Stage s = check_fwd(x, weight, bias, skip, G, eps, false);
  const auto o = x.options().memory_format(at::MemoryFormat::Contiguous);
  return {at::empty(s.out_sizes(), o), at::empty({s.B, s.G, 4}, o.dtype(at::kFloat))};
}

// the backward's own checks; x / weight / bias / stats may be None when only dskip is wanted
Stage check_bwd(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, bool nX, bool nW, bool nB,
                bool nS, bool device) {
  TORCH_CHECK(nX || nW || nB || nS, "sgrender: gn_stage_bwd: no gradient requested");
  TORCH_CHECK(!nS || Cs > 0, "sgrender: gn_stage_bwd: a skip gradient requested without skip channels");
  if (device) TORCH_CHECK(g.is_cuda(), kNoCpu);
  TORCH_CHECK(g.dim() == 4 && io_type(g.scalar_type()) && C > 0 && Cs >= 0 && g.size(1) == C + Cs, "sgrender: gn_stage_bwd: the cotangent must be fp32 or bf16 [B,",
              C + Cs, ",.,.], got ", g.scalar_type(), " ", g.sizes());
  Stage s;
  s.B = g.size(0); s.C = C; s.Cs = Cs; s.G = G;
  s.H = Cs > 0 ? g.size(2) / 2 : g.size(2);
  s.W = Cs > 0 ? g.size(3) / 2 : g.size(3);
  TORCH_CHECK(g.sizes() == at::IntArrayRef(s.out_sizes()), "sgrender: gn_stage_bwd: the cotangent of an upsampled result must have even sizes, got ", g.sizes());
  check_sizes(s);
  if (nX || nW || nB) {
    TORCH_CHECK(has(x) && has(weight) && has(bias) && has(stats), "sgrender: gn_stage_bwd: x, weight, bias and stats are needed for dx, dweight and dbias");
    if (device) TORCH_CHECK(x->is_cuda() && weight->is_cuda() && bias->is_cuda() && stats->is_cuda(), kNoCpu);
    TORCH_CHECK(!io_type(x->scalar_type()) || x->scalar_type() == g.scalar_type(), "sgrender: gn_stage_bwd: x and the cotangent must have one dtype, got x ",
                x->scalar_type(), " and the cotangent ", g.scalar_type());
    TORCH_CHECK(io_type(x->scalar_type()) && x->sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: gn_stage_bwd: x must be fp32 or bf16 [", s.B, ",", s.C, ",", s.H,
                ",", s.W, "], got ", x->scalar_type(), " ", x->sizes());
    TORCH_CHECK(weight->scalar_type() == at::kFloat && bias->scalar_type() == at::kFloat && weight->dim() == 1 && bias->dim() == 1 && weight->size(0) == s.C &&
                    bias->size(0) == s.C,
                "sgrender: gn_stage_bwd: weight and bias must be fp32 [", s.C, "]");
    TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->sizes() == at::IntArrayRef({s.B, s.G, 4}), "sgrender: gn_stage_bwd: stats must be fp32 [", s.B, ",", s.G,
                ",4], got ", stats->sizes());
  }
  return s;
}
// a [0] tensor where a gradient is not wanted; dx and dskip in the cotangent's dtype (o), dweight and dbias in fp32
T4 bwd_outputs(const Stage& s, const at::TensorOptions& o, bool nX, bool nW, bool nB, bool nS) {
  const auto of = o.dtype(at::kFloat);
  return {at::empty(nX ? std::vector<int64_t>{s.B, s.C, s.H, s.W} : std::vector<int64_t>{0}, o), at::empty({nW ? s.C : 0}, of), at::empty({nB ? s.C : 0}, of),
          at::empty(nS ? std::vector<int64_t>{s.B, s.Cs, s.H, s.W} : std::vector<int64_t>{0}, o)};
}
T4 gn_stage_bwd_cuda(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, bool nX, bool nW, bool nB,
                     bool nS) {
  const Stage s = check_bwd(g, x, weight, bias, stats, C, Cs, G, nX, nW, nB, nS, true);
  const c10::DeviceGuard guard(g.device());
  const auto o = g.options().memory_format(at::MemoryFormat::Contiguous);
  const bool side = nX || nW || nB;
  T4 out = bwd_outputs(s, o, nX, nW, nB, nS);
  const Tensor gc = g.contiguous();
  Tensor w, b, st, ws;
  Strides4 xs{};
  if (side) {
    w = weight->contiguous(); b = bias->contiguous(); st = stats->contiguous();
    ws = workspace(s, true, o.dtype(at::kFloat));
    xs = strides_of(*x);
  }
  if (g.scalar_type() == at::kBFloat16) {
    ok(api().sgr_gn_stage_bwd_bf16(hrp(gc), side ? hrp(*x) : nullptr, rp(w), rp(b), rp(st), hwp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)),
                                   hwp(std::get<3>(out)), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, side ? xs.v : nullptr,
                                   stream_of(g.device())),
       "sgr_gn_stage_bwd_bf16");
    return out;
  }
  ok(api().sgr_gn_stage_bwd(rp(gc), side ? rp(*x) : nullptr, rp(w), rp(b), rp(st), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)),
                            wp(std::get<3>(out)), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, side ? xs.v : nullptr, stream_of(g.device())),
     "sgr_gn_stage_bwd");
  return out;
}
T4 gn_stage_bwd_meta(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, bool nX, bool nW, bool nB,
                     bool nS) {
  const Stage s = check_bwd(g, x, weight, bias, stats, C, Cs, G, nX, nW, nB, nS, false);
  return bwd_outputs(s, g.options().memory_format(at::MemoryFormat::Contiguous), nX, nW, nB, nS);
}

using FwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const OT&, int64_t, double);
using BwdSig = T4(const Tensor&, const OT&, const OT&, const OT&, const OT&, int64_t, int64_t, int64_t, bool, bool, bool, bool);

struct GnStageFn : public torch::autograd::Function<GnStageFn> {
  static variable_list forward(AutogradContext* ctx, const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps, bool nX, bool nW,
                               bool nB, bool nS) {
    T2 out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::gn_stage");
      out = op.call(x, weight, bias, skip, G, eps);
    }
    // y is recomputed from x and the statistics; skip is not kept: its gradient is linear in the cotangent
    const bool side = nX || nW || nB;
    ctx->save_for_backward({side ? x : Tensor(), side ? weight : Tensor(), side ? bias : Tensor(), side ? std::get<1>(out) : Tensor()});
    ctx->saved_data["C"] = x.size(1);
    ctx->saved_data["Cs"] = has(skip) ? skip->size(1) : (int64_t)0;
    ctx->saved_data["G"] = G;
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB; ctx->saved_data["nS"] = nS;
    ctx->mark_non_differentiable({std::get<1>(out)});
    return {std::get<0>(out), std::get<1>(out)};
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(10);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    const bool need[4] = {ctx->saved_data["nX"].toBool(), ctx->saved_data["nW"].toBool(), ctx->saved_data["nB"].toBool(), ctx->saved_data["nS"].toBool()};
    static auto bwd = find_op<BwdSig>("sgrender::gn_stage_bwd");
    auto [dx, dw, db, ds] = bwd.call(g[0], opt_of(s[0]), opt_of(s[1]), opt_of(s[2]), opt_of(s[3]), ctx->saved_data["C"].toInt(), ctx->saved_data["Cs"].toInt(),
                                     ctx->saved_data["G"].toInt(), need[0], need[1], need[2], need[3]);
    if (need[0]) out[0] = dx;
    if (need[1]) out[1] = dw;
    if (need[2]) out[2] = db;
    if (need[3]) out[3] = ds;
    return out;
  }
};

T2 gn_stage_autograd(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps) {
  const bool grad = at::GradMode::is_enabled();
  const bool nX = grad && x.requires_grad(), nW = grad && weight.requires_grad(), nB = grad && bias.requires_grad(), nS = grad && has(skip) && skip->requires_grad();
  if (!(nX || nW || nB || nS)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::gn_stage");
    return op.call(x, weight, bias, skip, G, eps);
  }
  auto o = GnStageFn::apply(x, weight, bias, skip, G, eps, nX, nW, nB, nS);
  return {o[0], o[1]};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("gn_stage(Tensor x, Tensor weight, Tensor bias, Tensor? skip, int num_groups, float eps=1e-05) -> (Tensor, Tensor)");
  m.def("gn_stage_bwd(Tensor g, Tensor? x, Tensor? weight, Tensor? bias, Tensor? stats, int channels, int skip_channels, int num_groups, bool need_x, bool need_weight, "
        "bool need_bias, bool need_skip) -> (Tensor, Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("gn_stage", &gn_stage_cuda);
  m.impl("gn_stage_bwd", &gn_stage_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("gn_stage", &gn_stage_meta);
  m.impl("gn_stage_bwd", &gn_stage_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("gn_stage", &gn_stage_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"gn_stage", "gn_stage_bwd"}); }

// torch.ops.sgrender.brdf_heads / brdf_heads_bwd: the output activations of the four BRDF decoders (models.py:189-203 and the wrappers'
// 0.5 (x + 1)) as operators of the C++ torch extension.
//
// Same rules as sgr_torch.cpp: every operator checks its arguments, allocates its outputs with the caching allocator and calls the C ABI
// (sgr_brdf_heads_fwd / _bwd of include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.  The
// `Tensor?` conventions are those of sgr_torch_brdf.cpp: None = the term is absent, a [0] tensor stands for a result that is not there.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;

#define HEAD_ARGS const OT &x_albedo, const OT &x_normal, const OT &x_rough, const OT &x_depth
#define HEAD_PASS x_albedo, x_normal, x_rough, x_depth
#define HEAD_SCHEMA "Tensor? x_albedo, Tensor? x_normal, Tensor? x_rough, Tensor? x_depth"

constexpr int64_t kOutCh[4] = {3, 3, 1, 1};

struct Heads {
  Tensor x[4];      // contiguous copies (undefined = absent)
  int64_t B = 0, H = 0, W = 0;
  const Tensor& first() const { return x[0].defined() ? x[0] : x[1].defined() ? x[1] : x[2].defined() ? x[2] : x[3]; }
};

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Heads check_heads(HEAD_ARGS, bool device) {
  Heads h;
  const OT* in[4] = {&x_albedo, &x_normal, &x_rough, &x_depth};
  const char* name[4] = {"xAlbedo", "xNormal", "xRough", "xDepth"};
  const Tensor* ref = nullptr;
  for (int k = 0; k < 4 && !ref; ++k)
    if (has(*in[k])) ref = &in[k]->value();
  TORCH_CHECK(ref, "sgrender: brdf_heads: every decoder output is None");
  if (device) TORCH_CHECK(ref->is_cuda(), kNoCpu);
  TORCH_CHECK(ref->dim() == 4, "sgrender: brdf_heads: a decoder output must be [B,3,H,W], got ", ref->sizes());
  h.B = ref->size(0); h.H = ref->size(2); h.W = ref->size(3);
  TORCH_CHECK(h.B > 0 && h.H > 0 && h.W > 0, "sgrender: brdf_heads: zero-sized decoder output ", ref->sizes());
  for (int k = 0; k < 4; ++k) {
    if (!has(*in[k])) continue;
    const Tensor& t = in[k]->value();
    if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
    TORCH_CHECK(t.device() == ref->device(), "sgrender: brdf_heads: tensors on different devices (", ref->device(), " vs ", t.device(), ")");
    TORCH_CHECK(t.scalar_type() == at::kFloat, "sgrender: brdf_heads: fp32 tensors required, ", name[k], " is ", t.scalar_type());
    TORCH_CHECK(t.sizes() == at::IntArrayRef({h.B, 3, h.H, h.W}), "sgrender: brdf_heads: ", name[k], " must be [", h.B, ",3,", h.H, ",", h.W, "] (dconvFinal has three channels; ",
                "the decoder outputs share one size), got ", t.sizes());
    h.x[k] = t.contiguous();
  }
  return h;
}

// -> (albedo, normal, rough, depth); a [0] tensor for an absent term
T4 brdf_heads_cuda(HEAD_ARGS, bool unit) {
  const Heads h = check_heads(HEAD_PASS, true);
  const auto dev = h.first().device();
  const c10::DeviceGuard guard(dev);
  const auto o = h.first().options().memory_format(at::MemoryFormat::Contiguous);
  Tensor y[4];
  for (int k = 0; k < 4; ++k) y[k] = h.x[k].defined() ? at::empty({h.B, kOutCh[k], h.H, h.W}, o) : at::empty({0}, o);
  ok(api().sgr_brdf_heads_fwd(rp(h.x[0]), rp(h.x[1]), rp(h.x[2]), rp(h.x[3]), wp(y[0]), wp(y[1]), wp(y[2]), wp(y[3]), (int)h.B, (int)h.H, (int)h.W, unit, stream_of(dev)),
     "sgr_brdf_heads_fwd");
  return {y[0], y[1], y[2], y[3]};
}
T4 brdf_heads_meta(HEAD_ARGS, bool) {
  const Heads h = check_heads(HEAD_PASS, false);
  const auto o = h.first().options().memory_format(at::MemoryFormat::Contiguous);
  Tensor y[4];
  for (int k = 0; k < 4; ++k) y[k] = h.x[k].defined() ? at::empty({h.B, kOutCh[k], h.H, h.W}, o) : at::empty({0}, o);
  return {y[0], y[1], y[2], y[3]};
}

#define COT_ARGS const OT &g_albedo, const OT &g_normal, const OT &g_rough, const OT &g_depth
void check_bwd(const Heads& h, const OT* const (&g)[4], const bool (&need)[4], bool device) {
  const char* name[4] = {"albedo", "normal", "rough", "depth"};
  TORCH_CHECK(need[0] || need[1] || need[2] || need[3], "sgrender: brdf_heads_bwd: no gradient requested");
  for (int k = 0; k < 4; ++k) {
    TORCH_CHECK(!need[k] || h.x[k].defined(), "sgrender: brdf_heads_bwd: gradient requested for a decoder output that is None (", name[k], ")");
    if (!has(*g[k])) continue;
    const Tensor& t = g[k]->value();
    TORCH_CHECK(h.x[k].defined(), "sgrender: brdf_heads_bwd: cotangent for a decoder output that is None (", name[k], ")");
    if (device) TORCH_CHECK(t.is_cuda() && t.device() == h.first().device(), kNoCpu);
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.sizes() == at::IntArrayRef({h.B, kOutCh[k], h.H, h.W}), "sgrender: brdf_heads_bwd: the ", name[k],
                " cotangent must be fp32 [", h.B, ",", kOutCh[k], ",", h.H, ",", h.W, "], got ", t.scalar_type(), " ", t.sizes());
  }
}
// -> the four gradients [B,3,H,W]; a [0] tensor where not wanted.  A None cotangent is zero (NULL to the C ABI)
T4 brdf_heads_bwd_cuda(HEAD_ARGS, COT_ARGS, bool unit, bool nA, bool nN, bool nR, bool nD) {
  const Heads h = check_heads(HEAD_PASS, true);
  const OT* const g[4] = {&g_albedo, &g_normal, &g_rough, &g_depth};
  const bool need[4] = {nA, nN, nR, nD};
  check_bwd(h, g, need, true);
  const auto dev = h.first().device();
  const c10::DeviceGuard guard(dev);
  const auto o = h.first().options().memory_format(at::MemoryFormat::Contiguous);
  Tensor gc[4], gx[4];
  for (int k = 0; k < 4; ++k) {
    if (need[k] && has(*g[k])) gc[k] = g[k]->value().contiguous();
    gx[k] = need[k] ? at::empty({h.B, 3, h.H, h.W}, o) : at::empty({0}, o);
  }
  ok(api().sgr_brdf_heads_bwd(rp(h.x[0]), rp(h.x[1]), rp(h.x[2]), rp(h.x[3]), rp(gc[0]), rp(gc[1]), rp(gc[2]), rp(gc[3]), wp(gx[0]), wp(gx[1]), wp(gx[2]), wp(gx[3]), (int)h.B,
                              (int)h.H, (int)h.W, unit, stream_of(dev)),
     "sgr_brdf_heads_bwd");
  return {gx[0], gx[1], gx[2], gx[3]};
}
T4 brdf_heads_bwd_meta(HEAD_ARGS, COT_ARGS, bool, bool nA, bool nN, bool nR, bool nD) {
  const Heads h = check_heads(HEAD_PASS, false);
  const OT* const g[4] = {&g_albedo, &g_normal, &g_rough, &g_depth};
  const bool need[4] = {nA, nN, nR, nD};
  check_bwd(h, g, need, false);
  const auto o = h.first().options().memory_format(at::MemoryFormat::Contiguous);
  Tensor gx[4];
  for (int k = 0; k < 4; ++k) gx[k] = need[k] ? at::empty({h.B, 3, h.H, h.W}, o) : at::empty({0}, o);
  return {gx[0], gx[1], gx[2], gx[3]};
}

using FwdSig = T4(const OT&, const OT&, const OT&, const OT&, bool);
using BwdSig = T4(const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, bool, bool, bool, bool, bool);

struct BrdfHeadsFn : public torch::autograd::Function<BrdfHeadsFn> {
  static variable_list forward(AutogradContext* ctx, HEAD_ARGS, bool unit, bool nA, bool nN, bool nR, bool nD) {
    T4 out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      static auto op = find_op<FwdSig>("sgrender::brdf_heads");
      out = op.call(HEAD_PASS, unit);
    }
    // the backward recomputes tanh from x: the decoder outputs whose gradient is wanted are all that is kept
    auto keep = [](const OT& t, bool need) { return need ? *t : Tensor(); };
    ctx->save_for_backward({keep(x_albedo, nA), keep(x_normal, nN), keep(x_rough, nR), keep(x_depth, nD)});
    ctx->saved_data["unit"] = unit;
    ctx->set_materialize_grads(false);
    variable_list y = {std::get<0>(out), std::get<1>(out), std::get<2>(out), std::get<3>(out)};
    const bool need[4] = {nA, nN, nR, nD};
    variable_list dead;
    for (int k = 0; k < 4; ++k)
      if (!need[k]) dead.push_back(y[k]);
    ctx->mark_non_differentiable(dead);
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(9);
    const auto s = ctx->get_saved_variables();
    bool need[4], any = false;
    for (int k = 0; k < 4; ++k) {
      need[k] = s[k].defined();
      any = any || (need[k] && g[k].defined());
    }
    if (!any) return out;
    static auto bwd = find_op<BwdSig>("sgrender::brdf_heads_bwd");
    // an output nobody used arrives undefined and travels on as None: a zero cotangent through a NULL pointer
    auto cot = [&](int k) { return need[k] && g[k].defined() ? OT(g[k]) : OT(); };
    auto [gA, gN, gR, gD] = bwd.call(opt_of(s[0]), opt_of(s[1]), opt_of(s[2]), opt_of(s[3]), cot(0), cot(1), cot(2), cot(3), ctx->saved_data["unit"].toBool(), need[0], need[1], need[2],
                                     need[3]);
    if (need[0]) out[0] = gA;
    if (need[1]) out[1] = gN;
    if (need[2]) out[2] = gR;
    if (need[3]) out[3] = gD;
    return out;
  }
};

T4 brdf_heads_autograd(HEAD_ARGS, bool unit) {
  const bool grad = at::GradMode::is_enabled();
  auto rg = [&](const OT& t) { return grad && has(t) && t->requires_grad(); };
  const bool nA = rg(x_albedo), nN = rg(x_normal), nR = rg(x_rough), nD = rg(x_depth);
  if (!(nA || nN || nR || nD)) {      // nothing to differentiate: no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto op = find_op<FwdSig>("sgrender::brdf_heads");
    return op.call(HEAD_PASS, unit);
  }
  auto o = BrdfHeadsFn::apply(HEAD_PASS, unit, nA, nN, nR, nD);
  return {o[0], o[1], o[2], o[3]};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("brdf_heads(" HEAD_SCHEMA ", bool unit=True) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("brdf_heads_bwd(" HEAD_SCHEMA ", Tensor? g_albedo, Tensor? g_normal, Tensor? g_rough, Tensor? g_depth, bool unit, bool need_albedo, bool need_normal, bool need_rough, "
        "bool need_depth) -> (Tensor, Tensor, Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("brdf_heads", &brdf_heads_cuda);
  m.impl("brdf_heads_bwd", &brdf_heads_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("brdf_heads", &brdf_heads_meta);
  m.impl("brdf_heads_bwd", &brdf_heads_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("brdf_heads", &brdf_heads_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"brdf_heads", "brdf_heads_bwd"}); }

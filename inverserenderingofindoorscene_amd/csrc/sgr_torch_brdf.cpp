// torch.ops.sgrender.brdf_objective* / batch_ranking_loss*: the BRDF-stage training objectives as operators of the C++ torch extension.
//
// Same rules as sgr_torch.cpp: every operator checks its arguments, allocates outputs and workspace with the caching allocator and calls
// the C ABI (sgr_brdf_objective_* / sgr_ranking_loss_* of include/sgrender.h) on the current HIP stream; nothing here computes and nothing
// synchronises.  The index tensors of the ranking loss are converted to int32 with at::Tensor::to (plumbing).
//
//   brdf_objective_fwd        wrapperBRDF.py:109-130, wrapperNYU.py:97-111: coefficients, batch totals, the six reported values
//   brdf_objective_finalize   the values from rank-summed totals (sharded batches)
//   brdf_objective_bwd        the gradients of the four predictions for five upstream gradients read on the device
//   brdf_objective            forward + autograd node (five differentiable scalars)
//   batch_ranking_loss(_fwd/_bwd)   wrapperIIW.py:88-109 with models.BatchRankingLoss, the whole batch in one call
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;
using W4 = at::ArrayRef<double>;

// ---- the objective: argument checks shared by the device and the Meta kernels -----------------------------------------------------------
struct Planes {
  Tensor aP, aG, nP, nG, rP, rG, dP, dG, sB, sA, sD;      // contiguous copies (undefined = absent)
  int64_t B = 0, H = 0, W = 0;
  const Tensor& first() const { return aP.defined() ? aP : nP.defined() ? nP : rP.defined() ? rP : dP; }
};
#define PLANE_ARGS                                                                                                                                         \
  const OT &albedoPred, const OT &albedo, const OT &normalPred, const OT &normal, const OT &roughPred, const OT &rough, const OT &depthPred, const OT &depth, \
      const OT &segBRDF, const OT &segAll, const OT &segDepth
#define PLANE_PASS albedoPred, albedo, normalPred, normal, roughPred, rough, depthPred, depth, segBRDF, segAll, segDepth
#define PLANE_SCHEMA                                                                                                                                        \
  "Tensor? albedoPred, Tensor? albedo, Tensor? normalPred, Tensor? normal, Tensor? roughPred, Tensor? rough, Tensor? depthPred, Tensor? depth, Tensor? segBRDF, " \
  "Tensor? segAll, Tensor? segDepth"

Planes check_planes(PLANE_ARGS, bool device) {
  Planes p;
  const OT* pred[4] = {&albedoPred, &normalPred, &roughPred, &depthPred};
  const OT* gt[4] = {&albedo, &normal, &rough, &depth};
  const char* name[4] = {"albedo", "normal", "rough", "depth"};
  const int64_t ch[4] = {3, 3, 1, 1};
  const Tensor* ref = nullptr;
  for (int k = 0; k < 4; ++k) {
    TORCH_CHECK(has(*pred[k]) == has(*gt[k]), "sgrender: brdf_objective: the ", name[k], " prediction and its ground truth must be given (or None) together");
    if (has(*pred[k]) && !ref) ref = &pred[k]->value();
  }
  TORCH_CHECK(ref, "sgrender: brdf_objective: every term is None");
  TORCH_CHECK(ref->dim() == 4, "sgrender: brdf_objective: predictions must be [B,C,H,W], got ", ref->sizes());
  p.B = ref->size(0); p.H = ref->size(2); p.W = ref->size(3);
  TORCH_CHECK(p.B > 0 && p.H > 0 && p.W > 0, "sgrender: brdf_objective: zero-sized prediction ", ref->sizes());
  const auto dev = ref->device();
  auto take = [&](const OT& t, int64_t c, const char* what) -> Tensor {
    if (!has(t)) return Tensor();
    if (device) TORCH_CHECK(t->is_cuda(), kNoCpu);
    TORCH_CHECK(t->device() == dev, "sgrender: brdf_objective: tensors on different devices (", dev, " vs ", t->device(), ")");
    TORCH_CHECK(t->scalar_type() == at::kFloat, "sgrender: brdf_objective: fp32 tensors required, ", what, " is ", t->scalar_type());
    TORCH_CHECK(t->sizes() == at::IntArrayRef({p.B, c, p.H, p.W}), "sgrender: brdf_objective: ", what, " must be [", p.B, ",", c, ",", p.H, ",", p.W, "], got ", t->sizes());
    return t->contiguous();
  };
  if (device) TORCH_CHECK(ref->is_cuda(), kNoCpu);
  p.aP = take(albedoPred, ch[0], "albedoPred"); p.aG = take(albedo, ch[0], "albedoBatch");
  p.nP = take(normalPred, ch[1], "normalPred"); p.nG = take(normal, ch[1], "normalBatch");
  p.rP = take(roughPred, ch[2], "roughPred"); p.rG = take(rough, ch[2], "roughBatch");
  p.dP = take(depthPred, ch[3], "depthPred"); p.dG = take(depth, ch[3], "depthBatch");
  p.sB = take(segBRDF, 1, "segBRDFBatch"); p.sA = take(segAll, 1, "segAllBatch"); p.sD = take(segDepth, 1, "segDepthBatch");
  TORCH_CHECK(!(p.aP.defined() || p.rP.defined()) || p.sB.defined(), "sgrender: brdf_objective: segBRDFBatch is needed for the albedo / roughness terms");
  TORCH_CHECK(!(p.nP.defined() || p.dP.defined()) || p.sA.defined(), "sgrender: brdf_objective: segAllBatch is needed for the normal / depth terms");
  return p;
}
void check_weights(W4 w, double off) {
  TORCH_CHECK(w.size() == 4, "sgrender: brdf_objective: weights must be (albedo, normal, rough, depth), got ", w.size(), " values");
  TORCH_CHECK(off > 0.0, "sgrender: brdf_objective: depth_offset must be positive, got ", off);
}
#define PLANE_PTRS(p) rp(p.aP), rp(p.aG), rp(p.nP), rp(p.nG), rp(p.rP), rp(p.rG), rp(p.dP), rp(p.dG), rp(p.sB), rp(p.sA), rp(p.sD)

// -> (values [6] or [0], parts [8], coef [B,2])
T3 brdf_objective_fwd_cuda(PLANE_ARGS, W4 w, double off, bool finalize) {
  Planes p = check_planes(PLANE_PASS, true);
  check_weights(w, off);
  const auto dev = p.first().device();
  const c10::DeviceGuard guard(dev);
  const auto o = p.first().options();
  Tensor values = at::empty({finalize ? 6 : 0}, o), parts = at::empty({8}, o), coef = at::empty({p.B, 2}, o);
  const int nws = api().sgr_brdf_objective_workspace_floats((int)p.B);
  Tensor ws = at::empty({(int64_t)nws}, o);
  ok(api().sgr_brdf_objective_fwd(PLANE_PTRS(p), coef.data_ptr<float>(), parts.data_ptr<float>(), wp(values), ws.data_ptr<float>(), (int)p.B, (int)p.H, (int)p.W, (float)w[0],
                                  (float)w[1], (float)w[2], (float)w[3], (float)off, stream_of(dev)),
     "sgr_brdf_objective_fwd");
  return {values, parts, coef};
}
T3 brdf_objective_fwd_meta(PLANE_ARGS, W4 w, double off, bool finalize) {
  const Planes p = check_planes(PLANE_PASS, false);
  check_weights(w, off);
  const auto o = p.first().options();
  return {at::empty({finalize ? 6 : 0}, o), at::empty({8}, o), at::empty({p.B, 2}, o)};
}

void check_parts(const Tensor& parts) {
  TORCH_CHECK(parts.numel() == 8 && parts.scalar_type() == at::kFloat, "sgrender: brdf_objective: parts must hold the 8 fp32 batch totals, got ", parts.sizes());
}
Tensor brdf_objective_finalize_cuda(const Tensor& parts, W4 w) {
  TORCH_CHECK(parts.is_cuda(), kNoCpu);
  check_parts(parts);
  check_weights(w, 1.0);
  const auto dev = parts.device();
  const c10::DeviceGuard guard(dev);
  const Tensor pc = parts.contiguous();
  Tensor values = at::empty({6}, pc.options());
  ok(api().sgr_brdf_objective_finalize(pc.const_data_ptr<float>(), values.data_ptr<float>(), (float)w[0], (float)w[1], (float)w[2], (float)w[3], stream_of(dev)),
     "sgr_brdf_objective_finalize");
  return values;
}
Tensor brdf_objective_finalize_meta(const Tensor& parts, W4 w) {
  check_parts(parts);
  check_weights(w, 1.0);
  return at::empty({6}, parts.options());
}

// -> the four gradients (a [0] tensor where not wanted)
#define UP_ARGS const OT &g_total, const OT &g_albedo, const OT &g_normal, const OT &g_rough, const OT &g_depth
void check_bwd(const Planes& p, const Tensor& coef, const Tensor& parts, bool nA, bool nN, bool nR, bool nD) {
  check_parts(parts);
  TORCH_CHECK(coef.sizes() == at::IntArrayRef({p.B, 2}) && coef.scalar_type() == at::kFloat, "sgrender: brdf_objective_bwd: coef must be fp32 [", p.B, ",2], got ", coef.sizes());
  TORCH_CHECK(nA || nN || nR || nD, "sgrender: brdf_objective_bwd: no gradient requested");
  TORCH_CHECK((!nA || p.aP.defined()) && (!nN || p.nP.defined()) && (!nR || p.rP.defined()) && (!nD || p.dP.defined()),
              "sgrender: brdf_objective_bwd: gradient requested for a term that is None");
}
T4 brdf_objective_bwd_cuda(UP_ARGS, PLANE_ARGS, const Tensor& coef, const Tensor& parts, W4 w, double off, bool nA, bool nN, bool nR, bool nD) {
  Planes p = check_planes(PLANE_PASS, true);
  check_weights(w, off);
  check_bwd(p, coef, parts, nA, nN, nR, nD);
  const auto dev = p.first().device();
  const c10::DeviceGuard guard(dev);
  const OT* up[5] = {&g_total, &g_albedo, &g_normal, &g_rough, &g_depth};
  Tensor g[5];
  for (int k = 0; k < 5; ++k) {
    if (!has(*up[k])) continue;
    TORCH_CHECK(up[k]->value().is_cuda() && up[k]->value().device() == dev, kNoCpu);
    TORCH_CHECK(up[k]->value().numel() == 1 && up[k]->value().scalar_type() == at::kFloat, "sgrender: brdf_objective_bwd: upstream gradients must be fp32 scalars");
    g[k] = up[k]->value().contiguous();
  }
  TORCH_CHECK(coef.is_cuda() && parts.is_cuda(), kNoCpu);
  const Tensor cc = coef.contiguous(), pc = parts.contiguous();
  const auto o = p.first().options();
  Tensor gA = nA ? at::empty_like(p.aP) : at::empty({0}, o), gN = nN ? at::empty_like(p.nP) : at::empty({0}, o);
  Tensor gR = nR ? at::empty_like(p.rP) : at::empty({0}, o), gD = nD ? at::empty_like(p.dP) : at::empty({0}, o);
  ok(api().sgr_brdf_objective_bwd(rp(g[0]), rp(g[1]), rp(g[2]), rp(g[3]), rp(g[4]), PLANE_PTRS(p), cc.const_data_ptr<float>(), pc.const_data_ptr<float>(), wp(gA), wp(gN),
                                  wp(gR), wp(gD), (int)p.B, (int)p.H, (int)p.W, (float)w[0], (float)w[1], (float)w[2], (float)w[3], (float)off, stream_of(dev)),
     "sgr_brdf_objective_bwd");
  return {gA, gN, gR, gD};
}
T4 brdf_objective_bwd_meta(UP_ARGS, PLANE_ARGS, const Tensor& coef, const Tensor& parts, W4 w, double off, bool nA, bool nN, bool nR, bool nD) {
  const Planes p = check_planes(PLANE_PASS, false);
  check_weights(w, off);
  check_bwd(p, coef, parts, nA, nN, nR, nD);
  const auto o = p.first().options();
  return {nA ? at::empty_like(p.aP) : at::empty({0}, o), nN ? at::empty_like(p.nP) : at::empty({0}, o), nR ? at::empty_like(p.rP) : at::empty({0}, o),
          nD ? at::empty_like(p.dP) : at::empty({0}, o)};
}

using FwdSig = T3(const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, W4, double, bool);
using FinSig = Tensor(const Tensor&, W4);
using BwdSig = T4(const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&, const OT&,
                  const OT&, const OT&, const Tensor&, const Tensor&, W4, double, bool, bool, bool, bool);

// (total, albedoErr, normalErr, roughErr, depthErr, angleMean, coef, parts).  `parts_in` / `coef_in`: the rank-summed totals and this
// shard's coefficients of an earlier brdf_objective_fwd (sharded batches) -- then only the values are formed here.
T8 brdf_objective_impl(PLANE_ARGS, const OT& parts_in, const OT& coef_in, W4 w, double off) {
  static auto fwd = find_op<FwdSig>("sgrender::brdf_objective_fwd");
  static auto fin = find_op<FinSig>("sgrender::brdf_objective_finalize");
  TORCH_CHECK(has(parts_in) == has(coef_in), "sgrender: brdf_objective: parts and coef come together");
  Tensor values, parts, coef;
  if (has(parts_in)) {
    parts = *parts_in;
    coef = *coef_in;
    values = fin.call(parts, w);
  } else {
    std::tie(values, parts, coef) = fwd.call(PLANE_PASS, w, off, true);
  }
  return {values.select(0, 0), values.select(0, 1), values.select(0, 2), values.select(0, 3), values.select(0, 4), values.select(0, 5), coef, parts};
}

struct BrdfObjectiveFn : public torch::autograd::Function<BrdfObjectiveFn> {
  static variable_list forward(AutogradContext* ctx, PLANE_ARGS, const OT& parts_in, const OT& coef_in, std::vector<double> w, double off, bool nA, bool nN, bool nR,
                               bool nD) {
    at::AutoDispatchBelowADInplaceOrView guard;
    auto o = brdf_objective_impl(PLANE_PASS, parts_in, coef_in, w, off);
    auto u = [](const OT& t) { return has(t) ? *t : Tensor(); };
    ctx->save_for_backward({u(albedoPred), u(albedo), u(normalPred), u(normal), u(roughPred), u(rough), u(depthPred), u(depth), u(segBRDF), u(segAll), u(segDepth),
                            std::get<6>(o), std::get<7>(o)});
    ctx->saved_data["w"] = w;
    ctx->saved_data["off"] = off;
    ctx->saved_data["nA"] = nA;
    ctx->saved_data["nN"] = nN;
    ctx->saved_data["nR"] = nR;
    ctx->saved_data["nD"] = nD;
    variable_list out = {std::get<0>(o), std::get<1>(o), std::get<2>(o), std::get<3>(o), std::get<4>(o), std::get<5>(o), std::get<6>(o), std::get<7>(o)};
    ctx->mark_non_differentiable({out[5], out[6], out[7]});
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(19);
    bool any = false;
    for (int k = 0; k < 5; ++k) any = any || g[k].defined();
    if (!any) return out;
    const auto s = ctx->get_saved_variables();
    const auto w = ctx->saved_data["w"].toDoubleVector();
    const bool need[4] = {ctx->saved_data["nA"].toBool(), ctx->saved_data["nN"].toBool(), ctx->saved_data["nR"].toBool(), ctx->saved_data["nD"].toBool()};
    static auto bwd = find_op<BwdSig>("sgrender::brdf_objective_bwd");
    auto [gA, gN, gR, gD] = bwd.call(opt_of(g[0]), opt_of(g[1]), opt_of(g[2]), opt_of(g[3]), opt_of(g[4]), opt_of(s[0]), opt_of(s[1]), opt_of(s[2]), opt_of(s[3]), opt_of(s[4]), opt_of(s[5]), opt_of(s[6]),
                                     opt_of(s[7]), opt_of(s[8]), opt_of(s[9]), opt_of(s[10]), s[11], s[12], w, ctx->saved_data["off"].toDouble(), need[0], need[1], need[2], need[3]);
    if (need[0]) out[0] = gA;
    if (need[1]) out[2] = gN;
    if (need[2]) out[4] = gR;
    if (need[3]) out[6] = gD;
    return out;
  }
};

T8 brdf_objective_autograd(PLANE_ARGS, const OT& parts_in, const OT& coef_in, W4 w, double off) {
  const bool grad = at::GradMode::is_enabled();
  auto rg = [&](const OT& t) { return grad && has(t) && t->requires_grad(); };
  TORCH_CHECK(!(rg(albedo) || rg(normal) || rg(rough) || rg(depth) || rg(segBRDF) || rg(segAll) || rg(segDepth) || rg(parts_in) || rg(coef_in)),
              "sgrender: brdf_objective differentiates with respect to the four predictions only; a ground-truth tensor or a mask requires grad -- detach it");
  const bool nA = rg(albedoPred), nN = rg(normalPred), nR = rg(roughPred), nD = rg(depthPred);
  if (!(nA || nN || nR || nD)) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return brdf_objective_impl(PLANE_PASS, parts_in, coef_in, w, off);
  }
  auto o = BrdfObjectiveFn::apply(PLANE_PASS, parts_in, coef_in, std::vector<double>(w.begin(), w.end()), off, nA, nN, nR, nD);
  return {o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
}

// ---- the ranking objective -----------------------------------------------------------------------------------------------------------------
struct RankDims { int64_t B, H, W, Ne, Nd; };
#define RANK_ARGS \
  const Tensor &albedoPred, const Tensor &eqPoint, const Tensor &eqWeight, const Tensor &eqNum, const Tensor &darkerPoint, const Tensor &darkerWeight, const Tensor &darkerNum
#define RANK_PASS albedoPred, eqPoint, eqWeight, eqNum, darkerPoint, darkerWeight, darkerNum
#define RANK_SCHEMA "Tensor albedoPred, Tensor eqPoint, Tensor eqWeight, Tensor eqNum, Tensor darkerPoint, Tensor darkerWeight, Tensor darkerNum"
RankDims check_rank(RANK_ARGS, bool device) {
  TORCH_CHECK(albedoPred.dim() == 4 && albedoPred.size(1) == 3, "sgrender: batch_ranking_loss: albedoPred must be [B,3,H,W], got ", albedoPred.sizes());
  if (device) TORCH_CHECK(albedoPred.is_cuda(), kNoCpu);
  TORCH_CHECK(albedoPred.scalar_type() == at::kFloat, "sgrender: batch_ranking_loss: fp32 albedoPred required, got ", albedoPred.scalar_type());
  const int64_t B = albedoPred.size(0), H = albedoPred.size(2), W = albedoPred.size(3);
  TORCH_CHECK(B > 0 && H > 0 && W > 0, "sgrender: batch_ranking_loss: zero-sized albedoPred ", albedoPred.sizes());
  auto one = [&](const Tensor& pt, const Tensor& wt, const Tensor& num, const char* what) -> int64_t {
    for (const Tensor* t : {&pt, &wt, &num}) {
      if (device) TORCH_CHECK(t->is_cuda(), kNoCpu);
      TORCH_CHECK(t->device() == albedoPred.device(), "sgrender: batch_ranking_loss: tensors on different devices");
    }
    TORCH_CHECK(pt.dim() == 3 && pt.size(0) == B && pt.size(2) == 4, "sgrender: batch_ranking_loss: ", what, "Point must be [", B, ",N,4], got ", pt.sizes());
    TORCH_CHECK(pt.scalar_type() == at::kInt || pt.scalar_type() == at::kLong, "sgrender: batch_ranking_loss: ", what, "Point must be int32 or int64");
    TORCH_CHECK(wt.sizes() == at::IntArrayRef({B, pt.size(1)}) && wt.scalar_type() == at::kFloat, "sgrender: batch_ranking_loss: ", what, "Weight must be fp32 [", B, ",",
                pt.size(1), "], got ", wt.sizes());
    TORCH_CHECK(num.numel() == B && (num.scalar_type() == at::kInt || num.scalar_type() == at::kLong), "sgrender: batch_ranking_loss: ", what, "Num must be int32 or int64 [", B,
                "], got ", num.sizes());
    return pt.size(1);
  };
  const int64_t Ne = one(eqPoint, eqWeight, eqNum, "eq"), Nd = one(darkerPoint, darkerWeight, darkerNum, "darker");
  TORCH_CHECK(2 * (Ne + Nd) <= 4096, "sgrender: batch_ranking_loss: at most 2048 (padded) judgements per image, equal + darker; got ", Ne + Nd);
  return {B, H, W, Ne, Nd};
}
struct RankTensors { Tensor a, ep, ew, en, dp, dw, dn; };
RankTensors rank_tensors(RANK_ARGS) {
  return {albedoPred.contiguous(),       eqPoint.to(at::kInt).contiguous(),     eqWeight.contiguous(),    eqNum.to(at::kInt).contiguous(),
          darkerPoint.to(at::kInt).contiguous(), darkerWeight.contiguous(), darkerNum.to(at::kInt).contiguous()};
}
#define RANK_PTRS(t) \
  t.a.const_data_ptr<float>(), t.ep.const_data_ptr<int>(), t.ew.const_data_ptr<float>(), t.en.const_data_ptr<int>(), t.dp.const_data_ptr<int>(), t.dw.const_data_ptr<float>(), t.dn.const_data_ptr<int>()

Tensor ranking_fwd_cuda(RANK_ARGS, double tau) {      // -> [2] = (eqLoss, darkerLoss)
  const auto d = check_rank(RANK_PASS, true);
  const auto dev = albedoPred.device();
  const c10::DeviceGuard guard(dev);
  const auto t = rank_tensors(RANK_PASS);
  Tensor out = at::empty({2}, t.a.options()), ws = at::empty({(int64_t)api().sgr_ranking_loss_workspace_floats((int)d.B)}, t.a.options());
  ok(api().sgr_ranking_loss_fwd(RANK_PTRS(t), out.data_ptr<float>(), ws.data_ptr<float>(), (int)d.B, (int)d.H, (int)d.W, (int)d.Ne, (int)d.Nd, (float)tau, stream_of(dev)),
     "sgr_ranking_loss_fwd");
  return out;
}
Tensor ranking_fwd_meta(RANK_ARGS, double) {
  check_rank(RANK_PASS, false);
  return at::empty({2}, albedoPred.options());
}
Tensor ranking_bwd_cuda(const OT& g_eq, const OT& g_darker, RANK_ARGS, double tau) {
  const auto d = check_rank(RANK_PASS, true);
  const auto dev = albedoPred.device();
  const c10::DeviceGuard guard(dev);
  const auto t = rank_tensors(RANK_PASS);
  Tensor g[2];
  const OT* up[2] = {&g_eq, &g_darker};
  for (int k = 0; k < 2; ++k) {
    if (!has(*up[k])) continue;
    TORCH_CHECK(up[k]->value().is_cuda() && up[k]->value().device() == dev, kNoCpu);
    TORCH_CHECK(up[k]->value().numel() == 1 && up[k]->value().scalar_type() == at::kFloat, "sgrender: batch_ranking_loss_bwd: upstream gradients must be fp32 scalars");
    g[k] = up[k]->value().contiguous();
  }
  Tensor out = at::empty_like(t.a);
  ok(api().sgr_ranking_loss_bwd(rp(g[0]), rp(g[1]), RANK_PTRS(t), out.data_ptr<float>(), (int)d.B, (int)d.H, (int)d.W, (int)d.Ne, (int)d.Nd, (float)tau, stream_of(dev)),
     "sgr_ranking_loss_bwd");
  return out;
}
Tensor ranking_bwd_meta(const OT&, const OT&, RANK_ARGS, double) {
  check_rank(RANK_PASS, false);
  return at::empty(albedoPred.sizes(), albedoPred.options());
}

using RankFwdSig = Tensor(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, double);
using RankBwdSig = Tensor(const OT&, const OT&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, double);

T2 ranking_impl(RANK_ARGS, double tau) {
  static auto fwd = find_op<RankFwdSig>("sgrender::batch_ranking_loss_fwd");
  const Tensor out = fwd.call(RANK_PASS, tau);
  return {out.select(0, 0), out.select(0, 1)};
}
struct RankingFn : public torch::autograd::Function<RankingFn> {
  static variable_list forward(AutogradContext* ctx, RANK_ARGS, double tau) {
    at::AutoDispatchBelowADInplaceOrView guard;
    auto [e, d] = ranking_impl(RANK_PASS, tau);
    ctx->save_for_backward({RANK_PASS});
    ctx->saved_data["tau"] = tau;
    return {e, d};
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(8);
    if (!g[0].defined() && !g[1].defined()) return out;
    const auto s = ctx->get_saved_variables();
    static auto bwd = find_op<RankBwdSig>("sgrender::batch_ranking_loss_bwd");
    out[0] = bwd.call(g[0].defined() ? OT(g[0]) : OT(), g[1].defined() ? OT(g[1]) : OT(), s[0], s[1], s[2], s[3], s[4], s[5], s[6], ctx->saved_data["tau"].toDouble());
    return out;
  }
};
T2 ranking_autograd(RANK_ARGS, double tau) {
  const bool grad = at::GradMode::is_enabled();
  TORCH_CHECK(!(grad && (eqWeight.requires_grad() || darkerWeight.requires_grad())),
              "sgrender: batch_ranking_loss differentiates with respect to albedoPred only; a weight tensor requires grad -- detach it");
  if (!(grad && albedoPred.requires_grad())) {
    at::AutoDispatchBelowADInplaceOrView guard;
    return ranking_impl(RANK_PASS, tau);
  }
  auto o = RankingFn::apply(RANK_PASS, tau);
  return {o[0], o[1]};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("brdf_objective_fwd(" PLANE_SCHEMA ", float[] weights, float depth_offset, bool finalize) -> (Tensor, Tensor, Tensor)");
  m.def("brdf_objective_finalize(Tensor parts, float[] weights) -> Tensor");
  m.def("brdf_objective_bwd(Tensor? g_total, Tensor? g_albedo, Tensor? g_normal, Tensor? g_rough, Tensor? g_depth, " PLANE_SCHEMA
        ", Tensor coef, Tensor parts, float[] weights, float depth_offset, bool need_albedo, bool need_normal, bool need_rough, bool need_depth) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("brdf_objective(" PLANE_SCHEMA ", Tensor? parts, Tensor? coef, float[] weights, float depth_offset) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("batch_ranking_loss_fwd(" RANK_SCHEMA ", float tau) -> Tensor");
  m.def("batch_ranking_loss_bwd(Tensor? g_eq, Tensor? g_darker, " RANK_SCHEMA ", float tau) -> Tensor");
  m.def("batch_ranking_loss(" RANK_SCHEMA ", float tau) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("brdf_objective_fwd", &brdf_objective_fwd_cuda);
  m.impl("brdf_objective_finalize", &brdf_objective_finalize_cuda);
  m.impl("brdf_objective_bwd", &brdf_objective_bwd_cuda);
  m.impl("brdf_objective", &brdf_objective_impl);
  m.impl("batch_ranking_loss_fwd", &ranking_fwd_cuda);
  m.impl("batch_ranking_loss_bwd", &ranking_bwd_cuda);
  m.impl("batch_ranking_loss", &ranking_impl);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("brdf_objective_fwd", &brdf_objective_fwd_meta);
  m.impl("brdf_objective_finalize", &brdf_objective_finalize_meta);
  m.impl("brdf_objective_bwd", &brdf_objective_bwd_meta);
  m.impl("brdf_objective", &brdf_objective_impl);
  m.impl("batch_ranking_loss_fwd", &ranking_fwd_meta);
  m.impl("batch_ranking_loss_bwd", &ranking_bwd_meta);
  m.impl("batch_ranking_loss", &ranking_impl);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) {
  m.impl("brdf_objective", &brdf_objective_autograd);
  m.impl("batch_ranking_loss", &ranking_autograd);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) {
  register_no_cpu(m, {"brdf_objective_fwd", "brdf_objective_finalize", "brdf_objective_bwd", "brdf_objective", "batch_ranking_loss_fwd", "batch_ranking_loss_bwd",
                      "batch_ranking_loss"});
}

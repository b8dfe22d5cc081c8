// torch.autocast rules for torch.ops.sgrender.* (DESIGN.md section 8j): what an operator does with its floating tensors when it is called
// inside `with torch.autocast('cuda', dtype=...)`.  With autocast off the Autocast key is not in the dispatch set and nothing here runs.
//
//   fp32 policy   every functional operator but gn_stage / gn_stage_bwd and their sibling forms: floating tensors (optional ones and lists included) are cast to
//                 fp32 and the result is fp32 -- what PyTorch does for its own group_norm, losses and interpolate.  The render layer, the
//                 objectives, the solver, the heads and the exact-fp32 MFMA convolutions have fp32 kernels only.
//   gn_stage      a bf16 x stays bf16 and skip is cast to it (native bf16 kernels, sgr_gn_stage.hip); anything else -- an fp16 x under an
//                 fp16 autocast too -- is cast to fp32 with its skip.  weight and bias are cast to fp32 either way.
//   gn_stage_bwd  the same rule on (cotangent, x): bf16 stays when x (or, without x, the cotangent) is bf16.
//   gn_stage_siblings / _bwd   gn_stage's rule on the lists: bf16 stays when every x (without any x: every cotangent) is bf16.
//   fall through  operators that write into an argument (rescale_grads_, rescale_grads6_, allreduce_sum_, light_objective_stage2(_brdf):
//                 a cast copy would take the write) and those without a tensor argument: no kernel here, PyTorch's fall-through applies.
//
// Written with at::autocast::cached_cast under an ExcludeDispatchKeyGuard, as PyTorch's own rules are: the casts are ordinary differentiable
// `to` calls, so the gradients come back in the callers' dtypes.
#include <algorithm>

#include <ATen/autocast_mode.h>

#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;
using at::autocast::cached_cast;

constexpr auto kDev = c10::DeviceType::CUDA;
c10::DispatchKeySet autocast_keys() { return c10::DispatchKeySet(c10::DispatchKey::AutocastCUDA); }

// fp32 policy for any schema: the arguments are cast on the stack, then the operator is called again below the Autocast key
void autocast_fp32(const c10::OperatorHandle& op, torch::jit::Stack* stack) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(autocast_keys());
  const size_t n = op.schema().arguments().size(), base = stack->size() - n;
  for (size_t i = 0; i < n; ++i) {
    c10::IValue& v = (*stack)[base + i];
    if (v.isTensor()) {      // Tensor and a Tensor? that is given
      v = cached_cast(at::kFloat, v.toTensor(), kDev);
    } else if (v.isTensorList()) {
      const std::vector<Tensor> ts = v.toTensorVector();
      v = cached_cast(at::kFloat, at::TensorList(ts), kDev);      // as a TensorList: a std::vector would pick cached_cast's pass-through template
    }
  }
  op.callBoxed(stack);
}

using FwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const OT&, int64_t, double);
using BwdSig = T4(const Tensor&, const OT&, const OT&, const OT&, const OT&, int64_t, int64_t, int64_t, bool, bool, bool, bool);

at::ScalarType io_type_of(const Tensor& t) { return t.scalar_type() == at::kBFloat16 ? at::kBFloat16 : at::kFloat; }

T2 gn_stage_autocast(const Tensor& x, const Tensor& weight, const Tensor& bias, const OT& skip, int64_t G, double eps) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(autocast_keys());
  const at::ScalarType io = io_type_of(x);
  static auto op = find_op<FwdSig>("sgrender::gn_stage");
  return op.call(cached_cast(io, x, kDev), cached_cast(at::kFloat, weight, kDev), cached_cast(at::kFloat, bias, kDev), cached_cast(io, skip, kDev), G, eps);
}

T4 gn_stage_bwd_autocast(const Tensor& g, const OT& x, const OT& weight, const OT& bias, const OT& stats, int64_t C, int64_t Cs, int64_t G, bool nX, bool nW, bool nB,
                         bool nS) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(autocast_keys());
  const at::ScalarType io = io_type_of(x.has_value() && x->defined() ? *x : g);
  static auto op = find_op<BwdSig>("sgrender::gn_stage_bwd");
  return op.call(cached_cast(io, g, kDev), cached_cast(io, x, kDev), cached_cast(at::kFloat, weight, kDev), cached_cast(at::kFloat, bias, kDev),
                 cached_cast(at::kFloat, stats, kDev), C, Cs, G, nX, nW, nB, nS);
}

// the sibling forms of gn_stage (sgr_torch_gn_siblings.cpp): gn_stage's rule on lists -- bf16 stays when every x is bf16
using TL = at::TensorList;
using TV = std::vector<Tensor>;
using SibFwdSig = std::tuple<TV, Tensor>(TL, TL, TL, const Tensor&, int64_t, double);
using SibBwdSig = std::tuple<TV, TV, TV, Tensor>(TL, TL, TL, TL, const OT&, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, bool);

// the I/O type of a list: bf16 when it has a non-empty tensor and all of those are bf16
bool all_bf16(TL ts) {
  bool any = false;
  for (const Tensor& t : ts)
    if (t.defined() && t.numel()) {
      if (t.scalar_type() != at::kBFloat16) return false;
      any = true;
    }
  return any;
}

std::tuple<TV, Tensor> gn_stage_siblings_autocast(TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(autocast_keys());
  const at::ScalarType io = all_bf16(xs) ? at::kBFloat16 : at::kFloat;
  static auto op = find_op<SibFwdSig>("sgrender::gn_stage_siblings");
  return op.call(cached_cast(io, xs, kDev), cached_cast(at::kFloat, weights, kDev), cached_cast(at::kFloat, biases, kDev), cached_cast(io, skip, kDev), G, eps);
}

std::tuple<TV, TV, TV, Tensor> gn_stage_siblings_bwd_autocast(TL gs, TL xs, TL weights, TL biases, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W,
                                                              int64_t nX, int64_t nW, int64_t nB, bool nS) {
  c10::impl::ExcludeDispatchKeyGuard no_autocast(autocast_keys());
  const bool any_x = std::any_of(xs.begin(), xs.end(), [](const Tensor& t) { return t.defined() && t.numel() > 0; });
  const at::ScalarType io = all_bf16(any_x ? xs : gs) ? at::kBFloat16 : at::kFloat;
  static auto op = find_op<SibBwdSig>("sgrender::gn_stage_siblings_bwd");
  return op.call(cached_cast(io, gs, kDev), cached_cast(io, xs, kDev), cached_cast(at::kFloat, weights, kDev), cached_cast(at::kFloat, biases, kDev),
                 cached_cast(at::kFloat, stats, kDev), C, Cs, G, H, W, nX, nW, nB, nS);
}

// every functional operator with a tensor argument, file by file as they are defined
constexpr const char* kFp32Ops[] = {
    // sgr_torch.cpp
    "sg_to_env", "sg_to_env_bwd", "render_env", "render_env_bwd_env", "render_bwd_brdf", "fused_render", "fused_render_bwd_sg", "lsregress_coef",
    "lsregress_diffspec_coef", "render_loss", "render_loss_finalize", "render_loss_bwd", "recon_loss_parts", "recon_loss_bwd", "light_heads", "light_heads_bwd",
    "sg_shading", "light_albedo_scale", "light_encoder_input", "attach_grads", "light_objective_fwdbwd", "light_objective", "light_objective_stage1",
    "light_objective_stage3", "attach_grads6", "light_objective_brdf_fwdbwd", "light_objective_brdf", "comm_init",
    // sgr_torch_brdf.cpp
    "brdf_objective_fwd", "brdf_objective_finalize", "brdf_objective_bwd", "brdf_objective", "batch_ranking_loss_fwd", "batch_ranking_loss_bwd", "batch_ranking_loss",
    // sgr_torch_brdf_input.cpp, sgr_torch_brdf_heads.cpp, sgr_torch_bilateral.cpp
    "brdf_encoder_input", "brdf_heads", "brdf_heads_bwd", "bilateral_grid", "bilateral_solve_fwd", "bilateral_solve_bwd", "bilateral_solve",
    // sgr_torch_gn_resize.cpp, sgr_torch_gn_siblings.cpp (the resize form), sgr_torch_final_conv.cpp, sgr_torch_light_final_conv.cpp, sgr_torch_encoder_conv.cpp
    "gn_resize", "gn_resize_bwd", "gn_resize_siblings", "gn_resize_siblings_bwd", "final_conv", "final_conv_bwd", "light_final_conv", "light_final_conv_bwd", "encoder_conv", "encoder_conv_bwd",
    "encoder_conv_cat", "encoder_conv_cat_bwd",
    // sgr_torch_loader_prep.cpp (the uint8 inputs are no floating tensors: the casts pass them by)
    "loader_masks", "loader_scale_hdr", "loader_brdf_maps", "loader_envmaps",
    // sgr_torch_export.cpp
    "export_image", "export_env_mosaic", "export_env_hwc",
    // sgr_torch_real_loader.cpp (uint8, int32 and bool inputs are no floating tensors and the casts leave float64 alone: colour stays double)
    "nyu_prepare", "iiw_image",
    // sgr_torch_eval_metrics.cpp (bytes and integers pass the casts by; a bf16 prediction is widened to fp32, the kernels' only type)
    "eval_whdr", "eval_normal_angle", "eval_depth_log_rmse",
    // sgr_torch_pil_resize.cpp (bytes in, bytes out: the casts pass the only tensor by, so the rule is a fall-through in effect)
    "pil_resize",
};

}  // namespace

TORCH_LIBRARY_IMPL(sgrender, Autocast, m) {
  for (const char* name : kFp32Ops) m.impl(name, torch::CppFunction::makeFromBoxedFunction<&autocast_fp32>());
  m.impl("gn_stage", &gn_stage_autocast);
  m.impl("gn_stage_bwd", &gn_stage_bwd_autocast);
  m.impl("gn_stage_siblings", &gn_stage_siblings_autocast);
  m.impl("gn_stage_siblings_bwd", &gn_stage_siblings_bwd_autocast);
}

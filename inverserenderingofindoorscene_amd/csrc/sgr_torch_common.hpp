// What sgr_torch.cpp, sgr_torch_bilateral.cpp, sgr_torch_brdf.cpp, sgr_torch_brdf_input.cpp, sgr_torch_brdf_heads.cpp, sgr_torch_gn_stage.cpp, sgr_torch_gn_resize.cpp, sgr_torch_gn_siblings.cpp, sgr_torch_final_conv.cpp, sgr_torch_light_final_conv.cpp, sgr_torch_encoder_conv.cpp, sgr_torch_loader_prep.cpp, sgr_torch_export.cpp, sgr_torch_real_loader.cpp, sgr_torch_eval_metrics.cpp, sgr_torch_pil_resize.cpp, sgr_torch_comm.cpp and sgr_torch_autocast.cpp (one libsgrender_torch.so) share: the C ABI of libsgrender.so,
// resolved ONCE for the whole extension, and the few helpers every operator file needs around it.
//
// The C ABI stays the drop-in boundary: resolved with dlopen at first use ($SGR_LIB, else the libsgrender.so next to the extension's
// .so), so development builds of the kernel library can be A/B-ed under the same host layer, and a missing library is a loud error, not
// a silent fallback.  Importing the extension and running Meta kernels never loads it.  One load serves every operator family, so a
// library selected through $SGR_LIB must export EVERY symbol of SGR_API_LIST, not just those of the family called first -- which the
// ABI-version check implies anyway.  Everything is `inline` in a named namespace: one definition per shared object, not per file.
#pragma once

#include <dlfcn.h>

#include <cstdlib>
#include <initializer_list>
#include <string>
#include <tuple>

#include <ATen/ATen.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include "../../include/sgrender.h"

namespace sgr_host {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;
using OptTensor = std::optional<Tensor>;
using T2 = std::tuple<Tensor, Tensor>;
using T3 = std::tuple<Tensor, Tensor, Tensor>;
using T4 = std::tuple<Tensor, Tensor, Tensor, Tensor>;
using T5 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor>;
using T7 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;
using T8 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;

// every C entry point the extension calls
#define SGR_API_LIST(X)                                                                                                          \
  X(sgr_abi_version) X(sgr_last_error) X(sgr_dirs_floats) X(sgr_fill_direction_table) X(sgr_fill_view_vectors)                   \
  X(sgr_sg_to_env_fwd) X(sgr_render_env_fwd) X(sgr_fused_fwd_tan) X(sgr_sg_to_env_bwd) X(sgr_fused_bwd_sg)                       \
  X(sgr_render_env_bwd_env) X(sgr_render_bwd_brdf) X(sgr_loss_workspace_floats) X(sgr_render_loss_fwd)                           \
  X(sgr_render_loss_fwd_total) X(sgr_render_loss_fwd_total_grads) X(sgr_loss_finalize) X(sgr_objective_finalize)                 \
  X(sgr_render_loss_bwd_scaled) X(sgr_lsregress_coef) X(sgr_lsregress_diffspec_coef) X(sgr_sg_shading)                           \
  X(sgr_recon_workspace_floats) X(sgr_recon_loss_fwd) X(sgr_recon_loss_bwd) X(sgr_fused_recon_supported)                         \
  X(sgr_heads_prologue_supported) X(sgr_fused_recon_workspace_floats) X(sgr_fused_fwd_recon_seg) X(sgr_light_objective_fwd)      \
  X(sgr_light_heads_fwd) X(sgr_light_heads_bwd) X(sgr_rescale_inplace_flip) X(sgr_glue_workspace_floats)                         \
  X(sgr_light_albedo_scale) X(sgr_light_input_fwd) X(sgr_fused_bwd_recon_brdf) X(sgr_fused_bwd_recon_total_brdf)                 \
  X(sgr_bs_workspace_bytes) X(sgr_bs_grid_keys) X(sgr_bs_grid_build) X(sgr_bs_solve_fwd) X(sgr_bs_solve_bwd)                     \
  X(sgr_brdf_objective_workspace_floats) X(sgr_brdf_objective_fwd) X(sgr_brdf_objective_finalize) X(sgr_brdf_objective_bwd)      \
  X(sgr_ranking_loss_workspace_floats) X(sgr_ranking_loss_fwd) X(sgr_ranking_loss_bwd)         \
  X(sgr_brdf_input_workspace_floats) X(sgr_brdf_input_fwd) X(sgr_brdf_heads_fwd) X(sgr_brdf_heads_bwd)                          \
  X(sgr_gn_stage_workspace_floats) X(sgr_gn_stage_fwd) X(sgr_gn_stage_bwd) X(sgr_gn_stage_fwd_bf16) X(sgr_gn_stage_bwd_bf16)        \
  X(sgr_gn_resize_workspace_floats) X(sgr_gn_resize_fwd) X(sgr_gn_resize_bwd)                                                       \
  X(sgr_gn_stage_siblings_workspace_floats) X(sgr_gn_stage_siblings_fwd) X(sgr_gn_stage_siblings_bwd)                               \
  X(sgr_gn_stage_siblings_fwd_bf16) X(sgr_gn_stage_siblings_bwd_bf16)                                                               \
  X(sgr_gn_resize_siblings_workspace_floats) X(sgr_gn_resize_siblings_fwd) X(sgr_gn_resize_siblings_bwd)                            \
  X(sgr_gn_moments) X(sgr_final_conv_workspace_floats) X(sgr_final_conv_fwd) X(sgr_final_conv_bwd)                              \
  X(sgr_light_final_conv_workspace_floats) X(sgr_light_final_conv_fwd) X(sgr_light_final_conv_bwd)                        \
  X(sgr_encoder_conv_workspace_floats) X(sgr_encoder_conv_fwd) X(sgr_encoder_conv_bwd)                                    \
  X(sgr_encoder_conv_cat_fwd) X(sgr_encoder_conv_cat_bwd)                                                                     \
  X(sgr_loader_masks) X(sgr_loader_scale_hdr) X(sgr_loader_brdf_maps) X(sgr_loader_envmaps)                                  \
  X(sgr_export_image_workspace_floats) X(sgr_export_image) X(sgr_export_env_mosaic) X(sgr_export_env_hwc)         \
  X(sgr_nyu_prepare) X(sgr_iiw_image)                                                                                          \
  X(sgr_eval_whdr) X(sgr_eval_partials_doubles) X(sgr_eval_normal_angle) X(sgr_eval_depth_log_rmse)                              \
  X(sgr_pil_resize_table_ints) X(sgr_pil_resize_table) X(sgr_pil_resize_workspace_bytes) X(sgr_pil_resize_tiled_fits) X(sgr_pil_resize_route) X(sgr_pil_resize_u8)

struct Api {
#define SGR_DECL(name) decltype(&::name) name = nullptr;
  SGR_API_LIST(SGR_DECL)
#undef SGR_DECL
  std::string path;
};

inline const Api& api() {
  static const Api a = [] {
    Api r;
    const char* env = std::getenv("SGR_LIB");
    if (env && env[0]) {
      r.path = env;
    } else {
      Dl_info info{};
      TORCH_CHECK(dladdr(reinterpret_cast<void*>(&api), &info) && info.dli_fname, "sgrender: cannot locate the torch extension on disk");
      std::string self = info.dli_fname;
      const auto slash = self.find_last_of('/');
      r.path = (slash == std::string::npos ? std::string(".") : self.substr(0, slash)) + "/libsgrender.so";
    }
    void* h = dlopen(r.path.c_str(), RTLD_NOW | RTLD_LOCAL);
    TORCH_CHECK(h, "sgrender: cannot load ", r.path, " (", dlerror(), "): the HIP library has not been built -- run "
                "__graft_entry__.build() or `make -C inverserenderingofindoorscene_amd/csrc`.  This package has no CPU / PyTorch fallback.");
#define SGR_LOAD(name)                                                                     \
  r.name = reinterpret_cast<decltype(r.name)>(dlsym(h, #name));                            \
  TORCH_CHECK(r.name, "sgrender: ", r.path, " does not export " #name "; stale build?");
    SGR_API_LIST(SGR_LOAD)
#undef SGR_LOAD
    TORCH_CHECK(r.sgr_abi_version() == SGR_ABI_VERSION, "sgrender: ", r.path, " has ABI version ", r.sgr_abi_version(), ", this extension needs ",
                SGR_ABI_VERSION);
    return r;
  }();
  return a;
}

inline void ok(int rc, const char* what) {
  if (rc != 0) {
    const char* msg = api().sgr_last_error();
    TORCH_CHECK(false, "sgrender: ", what, " failed (code ", rc, "): ", msg ? msg : "");
  }
}

constexpr const char* kNoCpu =
    "sgrender: this layer runs only on HIP device tensors (MI355X); there is no CPU path. Move the inputs to the GPU (the reference's "
    "isCuda=True mode).";

// absent (undefined) and empty tensors are NULL to the C ABI
inline const float* rp(const Tensor& t) { return t.defined() && t.numel() ? t.const_data_ptr<float>() : nullptr; }
inline const float* rp(const Tensor* t) { return t ? rp(*t) : nullptr; }
inline float* wp(const Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }

inline void* stream_of(const c10::Device& dev) { return c10::hip::getCurrentHIPStream(dev.index()).stream(); }

// "given" for a tensor (defined and not empty) and for an optional one; an undefined saved tensor or cotangent as nullopt (autograd nodes)
inline bool present(const Tensor& t) { return t.defined() && t.numel() > 0; }
inline bool has(const OptTensor& t) { return t.has_value() && t->defined(); }
inline OptTensor opt_of(const Tensor& t) { return t.defined() ? OptTensor(t) : OptTensor(); }
// operators return tensors only: a [0] tensor where nothing is wanted
inline Tensor none(const at::TensorOptions& o) { return at::empty({0}, o); }
inline Tensor none_like(const Tensor& t) { return none(t.options()); }
// a 4-D map travels with its strides (channels-last maps and slices are not copied)
struct Strides4 { long long v[4]; };
inline Strides4 strides_of(const Tensor& t) { return {{(long long)t.stride(0), (long long)t.stride(1), (long long)t.stride(2), (long long)t.stride(3)}}; }
// a workspace of the n floats the C ABI asked for (n <= 0: it has no answer for these sizes)
inline Tensor workspace_floats(long long n, const char* who, const at::TensorOptions& o) {
  TORCH_CHECK(n > 0, "sgrender: ", who, ": no workspace size for these sizes");
  return at::empty({(int64_t)n}, o);
}

template <typename Sig>
auto find_op(const char* name) {
  return c10::Dispatcher::singleton().findSchemaOrThrow(name, "").typed<Sig>();
}

// no CPU path: every operator raises on CPU tensors (a namespace cannot carry a backend fallback, hence one registration each)
inline void no_cpu_path(const c10::OperatorHandle&, torch::jit::Stack*) { TORCH_CHECK(false, kNoCpu); }
inline void register_no_cpu(torch::Library& m, std::initializer_list<const char*> names) {
  for (const char* name : names) m.impl(name, torch::CppFunction::makeFromBoxedFunction<&no_cpu_path>());
}

}  // namespace sgr_host

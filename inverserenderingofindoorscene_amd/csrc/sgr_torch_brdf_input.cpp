// torch.ops.sgrender.brdf_encoder_input: the cascade-1 BRDF encoder's input (wrapperBRDF.py:56-100) as an operator of the C++ torch
// extension.
//
// Same rules as sgr_torch.cpp: the operator checks its arguments, allocates the outputs and the workspace with the caching allocator and
// calls the C ABI (sgr_brdf_input_fwd of include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.
// Forward only: every input is data in the reference, so there is no autograd node.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

struct InDims { int64_t bn, H, W, h, w, R, C; };

bool size_legal(int64_t h, int64_t w, int64_t H, int64_t W) { return (h == H && w == W) || h < H || w < W; }

// shared by the device and the Meta kernel: a traced graph cannot pass tracing and then fail on the device
InDims check_inputs(const Tensor& im, const Tensor& albedo, const Tensor& normal, const Tensor& rough, const Tensor& depth, const Tensor& diffuse, const Tensor& spec,
                    bool device) {
  const Tensor* all[7] = {&im, &albedo, &normal, &rough, &depth, &diffuse, &spec};
  const char* name[7] = {"imBatch", "albedoPre", "normalPre", "roughPre", "depthPre", "diffusePre", "specularPre"};
  const int64_t ch[7] = {3, 3, 3, 1, 1, 3, 3};
  for (int k = 0; k < 7; ++k) {
    if (device) TORCH_CHECK(all[k]->is_cuda(), kNoCpu);
    TORCH_CHECK(all[k]->device() == im.device(), "sgrender: brdf_encoder_input: tensors on different devices (", im.device(), " vs ", all[k]->device(), ")");
    TORCH_CHECK(all[k]->scalar_type() == at::kFloat, "sgrender: brdf_encoder_input: fp32 tensors required, ", name[k], " is ", all[k]->scalar_type());
    TORCH_CHECK(all[k]->dim() == 4 && all[k]->size(0) == im.size(0) && all[k]->size(1) == ch[k], "sgrender: brdf_encoder_input: ", name[k], " must be [", im.size(0), ",",
                ch[k], ",*,*], got ", all[k]->sizes());
    TORCH_CHECK(all[k]->numel() > 0, "sgrender: brdf_encoder_input: zero-sized ", name[k], " ", all[k]->sizes());
  }
  const InDims d{im.size(0), im.size(2), im.size(3), albedo.size(2), albedo.size(3), diffuse.size(2), diffuse.size(3)};
  for (int k = 2; k < 5; ++k)
    TORCH_CHECK(all[k]->size(2) == d.h && all[k]->size(3) == d.w, "sgrender: brdf_encoder_input: albedoPre, normalPre, roughPre and depthPre must share one size (", d.h, "x",
                d.w, "), ", name[k], " is ", all[k]->sizes());
  TORCH_CHECK(spec.size(2) == d.R && spec.size(3) == d.C, "sgrender: brdf_encoder_input: diffusePre and specularPre must share one size, got ", diffuse.sizes(), " and ",
              spec.sizes());
  TORCH_CHECK(size_legal(d.h, d.w, d.H, d.W), "sgrender: brdf_encoder_input: the BRDF maps (", d.h, "x", d.w, ") must have the image's size (", d.H, "x", d.W,
              ") or be smaller along an axis");
  TORCH_CHECK(size_legal(d.R, d.C, d.H, d.W), "sgrender: brdf_encoder_input: diffusePre / specularPre (", d.R, "x", d.C, ") must have the image's size (", d.H, "x", d.W,
              ") or be smaller along an axis");
  return d;
}

// -> (inputBatch [bn,17,H,W], coef [bn,2])
T2 brdf_encoder_input_cuda(const Tensor& im, const Tensor& albedo, const Tensor& normal, const Tensor& rough, const Tensor& depth, const Tensor& diffuse, const Tensor& spec,
                           bool regress, bool normalize, bool remap) {
  const InDims d = check_inputs(im, albedo, normal, rough, depth, diffuse, spec, true);
  const auto dev = im.device();
  const c10::DeviceGuard guard(dev);
  const Tensor i = im.contiguous(), a = albedo.contiguous(), n = normal.contiguous(), r = rough.contiguous(), dp = depth.contiguous(), df = diffuse.contiguous(),
               sp = spec.contiguous();
  const auto o = i.options().memory_format(at::MemoryFormat::Contiguous);
  Tensor out = at::empty({d.bn, 17, d.H, d.W}, o), coef = at::empty({d.bn, 2}, o);
  Tensor ws = at::empty({(int64_t)api().sgr_brdf_input_workspace_floats((int)d.bn)}, o);
  ok(api().sgr_brdf_input_fwd(rp(i), rp(a), rp(n), rp(r), rp(dp), rp(df), rp(sp), wp(out), wp(coef), wp(ws), (int)d.bn, (int)d.H, (int)d.W, (int)d.h, (int)d.w, (int)d.R,
                              (int)d.C, regress, normalize, remap, stream_of(dev)),
     "sgr_brdf_input_fwd");
  return {out, coef};
}
T2 brdf_encoder_input_meta(const Tensor& im, const Tensor& albedo, const Tensor& normal, const Tensor& rough, const Tensor& depth, const Tensor& diffuse, const Tensor& spec,
                           bool, bool, bool) {
  const InDims d = check_inputs(im, albedo, normal, rough, depth, diffuse, spec, false);
  const auto o = im.options().memory_format(at::MemoryFormat::Contiguous);
  return {at::empty({d.bn, 17, d.H, d.W}, o), at::empty({d.bn, 2}, o)};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("brdf_encoder_input(Tensor im, Tensor albedo, Tensor normal, Tensor rough, Tensor depth, Tensor diffuse, Tensor spec, bool regress=True, bool normalize=True, "
        "bool remap=False) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) { m.impl("brdf_encoder_input", &brdf_encoder_input_cuda); }
TORCH_LIBRARY_IMPL(sgrender, Meta, m) { m.impl("brdf_encoder_input", &brdf_encoder_input_meta); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"brdf_encoder_input"}); }

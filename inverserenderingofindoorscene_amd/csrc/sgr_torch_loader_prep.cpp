// torch.ops.sgrender.loader_*: the synthetic loader's batch preparation (dataLoader.py:118-154, 251-259, 286-310) as operators of the C++
// torch extension.
//
// Same rules as sgr_torch.cpp: an operator checks its arguments -- one check shared by the device and the Meta kernel, so that a traced graph
// cannot pass tracing and then fail on the device --, allocates the outputs with the caching allocator and calls the C ABI (sgr_loader_* of
// include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.  The results are inputs of the training
// step: no autograd node.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

constexpr const char* kMaskNumpy =
    "; on the host it is 0.5 * ((u8 - 127.5) / 127.5 + 1), three comparisons and scipy.ndimage.binary_erosion(segObj, np.ones((7, 7)), border_value=1)";
constexpr const char* kScaleNumpy = "; on the host it is np.sort((hdr * seg).flatten())[k], scale = (0.95 - 0.1 u) / max(v, 0.1), np.clip(scale * hdr, 0, 1)[::-1]";
constexpr const char* kMapsNumpy =
    "; on the host it is (0.5 * ((u8 - 127.5) / 127.5 + 1)) ** 2.2, n / np.sqrt(np.maximum(np.sum(n * n, axis=0), 1e-5)) and ((u8 - 127.5) / 127.5)[0:1]";
constexpr const char* kEnvNumpy =
    "; on the host it is env.reshape(R, 16, C, 32, 3).transpose(4, 0, 2, 1, 3), np.ascontiguousarray, the mean over non-overlapping blocks, times scale";

const unsigned char* bp(const Tensor& t) { return t.const_data_ptr<uint8_t>(); }

// a [bn,H,W,c] tensor of `type` with 1 <= c <= cmax (cmin == cmax: exactly that many)
void check_hwc(const Tensor& t, at::ScalarType type, int64_t cmin, int64_t cmax, const char* op, const char* name, const char* numpy, bool device) {
  if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
  TORCH_CHECK(t.scalar_type() == type, "sgrender: ", op, ": ", name, " must be ", type, ", got ", t.scalar_type(), numpy);
  TORCH_CHECK(t.dim() == 4 && t.size(3) >= cmin && t.size(3) <= cmax, "sgrender: ", op, ": ", name, " must be [bn,H,W,c] with ", cmin, " <= c <= ", cmax,
              " (the layout the file readers hand over), got ", t.sizes(), numpy);
  TORCH_CHECK(t.numel() > 0, "sgrender: ", op, ": zero-sized ", name, " ", t.sizes());
  TORCH_CHECK(t.size(0) <= 65535 && t.size(1) * t.size(2) < (int64_t(1) << 28), "sgrender: ", op, ": ", name, " ", t.sizes(), " is out of range (bn <= 65535, H W < 2^28)", numpy);
}
void check_same(const Tensor& t, const Tensor& ref, const char* op, const char* name, const char* ref_name) {
  TORCH_CHECK(t.device() == ref.device(), "sgrender: ", op, ": tensors on different devices (", ref.device(), " vs ", t.device(), ")");
  TORCH_CHECK(t.size(0) == ref.size(0) && t.size(1) == ref.size(1) && t.size(2) == ref.size(2), "sgrender: ", op, ": ", name, " ", t.sizes(), " and ", ref_name, " ", ref.sizes(),
              " must share [bn,H,W]");
}
void check_per_image(const Tensor& t, int64_t bn, const Tensor& ref, const char* op, const char* name, bool device) {
  if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
  TORCH_CHECK(t.device() == ref.device(), "sgrender: ", op, ": tensors on different devices (", ref.device(), " vs ", t.device(), ")");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "sgrender: ", op, ": ", name, " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.numel() == bn, "sgrender: ", op, ": ", name, " must hold one value per image (", bn, "), got ", t.sizes());
}
at::TensorOptions f32(const Tensor& like) { return like.options().dtype(at::kFloat).memory_format(at::MemoryFormat::Contiguous); }

// ---- masks ----------------------------------------------------------------------------------------------------------------------------
void masks_check(const Tensor& seg, bool device) { check_hwc(seg, at::kByte, 1, 4, "loader_masks", "seg_u8", kMaskNumpy, device); }
T3 masks_alloc(const Tensor& seg) {
  const auto o = f32(seg);
  const std::vector<int64_t> shape{seg.size(0), 1, seg.size(1), seg.size(2)};
  return {at::empty(shape, o), at::empty(shape, o), at::empty(shape, o)};
}
T3 loader_masks_cuda(const Tensor& seg, bool erode) {
  masks_check(seg, true);
  const c10::DeviceGuard guard(seg.device());
  const Tensor s = seg.contiguous();
  T3 out = masks_alloc(s);
  ok(api().sgr_loader_masks(bp(s), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), (int)s.size(0), (int)s.size(1), (int)s.size(2), (int)s.size(3), erode,
                            stream_of(seg.device())),
     "sgr_loader_masks");
  return out;
}
T3 loader_masks_meta(const Tensor& seg, bool) {
  masks_check(seg, false);
  return masks_alloc(seg);
}

// ---- HDR scale ------------------------------------------------------------------------------------------------------------------------
void scale_check(const Tensor& hdr, const Tensor& seg, const OptTensor& num, int64_t k, bool device) {
  check_hwc(hdr, at::kFloat, 3, 3, "loader_scale_hdr", "hdr", kScaleNumpy, device);
  check_hwc(seg, at::kByte, 1, 4, "loader_scale_hdr", "seg_u8", kScaleNumpy, device);
  check_same(seg, hdr, "loader_scale_hdr", "seg_u8", "hdr");
  if (has(num)) check_per_image(*num, hdr.size(0), hdr, "loader_scale_hdr", "num", device);
  TORCH_CHECK(k >= 0 && k < 3 * hdr.size(1) * hdr.size(2), "sgrender: loader_scale_hdr: the rank k = ", k, " must lie in [0, 3 H W = ", 3 * hdr.size(1) * hdr.size(2), ")");
}
T3 scale_alloc(const Tensor& hdr) {
  const auto o = f32(hdr);
  return {at::empty({hdr.size(0), 3, hdr.size(1), hdr.size(2)}, o), at::empty({hdr.size(0)}, o), at::empty({hdr.size(0)}, o)};
}
// -> (im [bn,3,H,W], scale [bn], v [bn])
T3 loader_scale_hdr_cuda(const Tensor& hdr, const Tensor& seg, const OptTensor& num, int64_t k) {
  scale_check(hdr, seg, num, k, true);
  const c10::DeviceGuard guard(hdr.device());
  const Tensor h = hdr.contiguous(), s = seg.contiguous();
  const Tensor n = has(num) ? num->contiguous() : Tensor();
  T3 out = scale_alloc(h);
  ok(api().sgr_loader_scale_hdr(rp(h), bp(s), rp(n), wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), (int)h.size(0), (int)h.size(1), (int)h.size(2),
                                (int)s.size(3), (long long)k, stream_of(hdr.device())),
     "sgr_loader_scale_hdr");
  return out;
}
T3 loader_scale_hdr_meta(const Tensor& hdr, const Tensor& seg, const OptTensor& num, int64_t k) {
  scale_check(hdr, seg, num, k, false);
  return scale_alloc(hdr);
}

// ---- BRDF maps --------------------------------------------------------------------------------------------------------------------------
const Tensor* maps_check(const OptTensor& albedo, const OptTensor& normal, const OptTensor& rough, bool device) {
  const Tensor* first = has(albedo) ? &*albedo : has(normal) ? &*normal : has(rough) ? &*rough : nullptr;
  TORCH_CHECK(first, "sgrender: loader_brdf_maps: at least one of albedo_u8, normal_u8, rough_u8 is needed");
  if (has(albedo)) check_hwc(*albedo, at::kByte, 3, 3, "loader_brdf_maps", "albedo_u8", kMapsNumpy, device);
  if (has(normal)) check_hwc(*normal, at::kByte, 3, 3, "loader_brdf_maps", "normal_u8", kMapsNumpy, device);
  if (has(rough)) check_hwc(*rough, at::kByte, 1, 4, "loader_brdf_maps", "rough_u8", kMapsNumpy, device);
  if (has(normal)) check_same(*normal, *first, "loader_brdf_maps", "normal_u8", "the first map");
  if (has(rough)) check_same(*rough, *first, "loader_brdf_maps", "rough_u8", "the first map");
  return first;
}
T3 maps_alloc(const OptTensor& albedo, const OptTensor& normal, const OptTensor& rough, const Tensor& first) {
  const auto o = f32(first);
  const int64_t bn = first.size(0), H = first.size(1), W = first.size(2);
  return {has(albedo) ? at::empty({bn, 3, H, W}, o) : none(o), has(normal) ? at::empty({bn, 3, H, W}, o) : none(o), has(rough) ? at::empty({bn, 1, H, W}, o) : none(o)};
}
// -> (albedo [bn,3,H,W], normal [bn,3,H,W], rough [bn,1,H,W]); a [0] tensor for a map that was not given
T3 loader_brdf_maps_cuda(const OptTensor& albedo, const OptTensor& normal, const OptTensor& rough) {
  const Tensor& first = *maps_check(albedo, normal, rough, true);
  const c10::DeviceGuard guard(first.device());
  const Tensor a = has(albedo) ? albedo->contiguous() : Tensor(), n = has(normal) ? normal->contiguous() : Tensor(), r = has(rough) ? rough->contiguous() : Tensor();
  T3 out = maps_alloc(albedo, normal, rough, first);
  ok(api().sgr_loader_brdf_maps(a.defined() ? bp(a) : nullptr, n.defined() ? bp(n) : nullptr, r.defined() ? bp(r) : nullptr, wp(std::get<0>(out)), wp(std::get<1>(out)),
                                wp(std::get<2>(out)), (int)first.size(0), (int)first.size(1), (int)first.size(2), r.defined() ? (int)r.size(3) : 1, stream_of(first.device())),
     "sgr_loader_brdf_maps");
  return out;
}
T3 loader_brdf_maps_meta(const OptTensor& albedo, const OptTensor& normal, const OptTensor& rough) {
  return maps_alloc(albedo, normal, rough, *maps_check(albedo, normal, rough, false));
}

// ---- env maps ---------------------------------------------------------------------------------------------------------------------------
void env_check(const Tensor& raw, const Tensor& scale, const OptTensor& ind, int64_t eh, int64_t ew, bool device) {
  if (device) TORCH_CHECK(raw.is_cuda(), kNoCpu);
  TORCH_CHECK(raw.scalar_type() == at::kFloat, "sgrender: loader_envmaps: env_raw must be fp32, got ", raw.scalar_type(), kEnvNumpy);
  TORCH_CHECK((eh == 8 && ew == 16) || (eh == 16 && ew == 32), "sgrender: loader_envmaps: envHeight x envWidth = ", eh, " x ", ew,
              " is not served: the file's cells are 16 x 32 and the ratio must be 2 (8 x 16) or 1 (16 x 32)", kEnvNumpy);
  TORCH_CHECK(raw.dim() == 4 && raw.size(3) == 3 && raw.numel() > 0 && raw.size(1) % 16 == 0 && raw.size(2) % 32 == 0, "sgrender: loader_envmaps: env_raw must be [bn, R * 16, C * 32, 3], got ",
              raw.sizes(), kEnvNumpy);
  TORCH_CHECK(raw.size(0) <= 65535 && raw.size(1) / 16 <= 65535 && raw.size(2) / 32 <= 65535, "sgrender: loader_envmaps: env_raw ", raw.sizes(), " is out of range (bn, R, C <= 65535)",
              kEnvNumpy);
  check_per_image(scale, raw.size(0), raw, "loader_envmaps", "scale", device);
  if (has(ind)) check_per_image(*ind, raw.size(0), raw, "loader_envmaps", "env_ind", device);
}
Tensor env_alloc(const Tensor& raw, int64_t eh, int64_t ew) { return at::empty({raw.size(0), 3, raw.size(1) / 16, raw.size(2) / 32, eh, ew}, f32(raw)); }
Tensor aligned_contiguous(const Tensor& t) {
  const Tensor c = t.contiguous();
  return (reinterpret_cast<uintptr_t>(c.const_data_ptr()) & 15) ? c.clone() : c;      // a view into a larger buffer may start anywhere
}
Tensor loader_envmaps_cuda(const Tensor& raw, const Tensor& scale, const OptTensor& ind, int64_t eh, int64_t ew) {
  env_check(raw, scale, ind, eh, ew, true);
  const c10::DeviceGuard guard(raw.device());
  const Tensor x = aligned_contiguous(raw), s = scale.contiguous(), i = has(ind) ? ind->contiguous() : Tensor();
  Tensor out = env_alloc(x, eh, ew);
  ok(api().sgr_loader_envmaps(rp(x), rp(s), rp(i), wp(out), (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)eh, (int)ew, stream_of(raw.device())), "sgr_loader_envmaps");
  return out;
}
Tensor loader_envmaps_meta(const Tensor& raw, const Tensor& scale, const OptTensor& ind, int64_t eh, int64_t ew) {
  env_check(raw, scale, ind, eh, ew, false);
  return env_alloc(raw, eh, ew);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("loader_masks(Tensor seg_u8, bool erode=True) -> (Tensor, Tensor, Tensor)");
  m.def("loader_scale_hdr(Tensor hdr, Tensor seg_u8, Tensor? num, int k) -> (Tensor, Tensor, Tensor)");
  m.def("loader_brdf_maps(Tensor? albedo_u8, Tensor? normal_u8, Tensor? rough_u8) -> (Tensor, Tensor, Tensor)");
  m.def("loader_envmaps(Tensor env_raw, Tensor scale, Tensor? env_ind=None, int envHeight=8, int envWidth=16) -> Tensor");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("loader_masks", &loader_masks_cuda);
  m.impl("loader_scale_hdr", &loader_scale_hdr_cuda);
  m.impl("loader_brdf_maps", &loader_brdf_maps_cuda);
  m.impl("loader_envmaps", &loader_envmaps_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("loader_masks", &loader_masks_meta);
  m.impl("loader_scale_hdr", &loader_scale_hdr_meta);
  m.impl("loader_brdf_maps", &loader_brdf_maps_meta);
  m.impl("loader_envmaps", &loader_envmaps_meta);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"loader_masks", "loader_scale_hdr", "loader_brdf_maps", "loader_envmaps"}); }

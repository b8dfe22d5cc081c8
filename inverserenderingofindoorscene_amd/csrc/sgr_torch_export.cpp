// torch.ops.sgrender.export_*: testReal's output stage and the image writers (testReal.py:542-657, utils.py:65-76, 102-154) as operators of
// the C++ torch extension.
//
// Same rules as sgr_torch.cpp: an operator checks its arguments -- one check shared by the device and the Meta kernel, so that a traced graph
// cannot pass tracing and then fail on the device --, allocates the outputs with the caching allocator and calls the C ABI (sgr_export_* of
// include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.  The results go to the file writers: no
// autograd node.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

constexpr int64_t kKinds = 8;
constexpr const char* kKindNames[kKinds] = {"albedo", "normal", "rough", "depth", "rendered", "shading", "image", "image_gamma"};
bool kind_resizes(int64_t kind) { return kind <= SGR_EXPORT_RENDERED; }
bool kind_takes(int64_t kind, int64_t C) {
  return (kind == SGR_EXPORT_ROUGH || kind == SGR_EXPORT_DEPTH) ? C == 1 : kind >= SGR_EXPORT_IMAGE ? (C == 1 || C == 3) : C == 3;
}
const char* kind_channels(int64_t kind) { return (kind == SGR_EXPORT_ROUGH || kind == SGR_EXPORT_DEPTH) ? "1" : kind >= SGR_EXPORT_IMAGE ? "1 or 3" : "3"; }

at::TensorOptions u8(const Tensor& like) { return like.options().dtype(at::kByte).memory_format(at::MemoryFormat::Contiguous); }
unsigned char* bwp(const Tensor& t) { return t.data_ptr<uint8_t>(); }

// ---- images -----------------------------------------------------------------------------------------------------------------------------
// -> (nh, nw)
std::pair<int64_t, int64_t> image_check(const Tensor& x, int64_t kind, at::OptionalIntArrayRef size, const OptTensor& scale, bool device) {
  if (device) TORCH_CHECK(x.is_cuda(), kNoCpu);
  TORCH_CHECK(kind >= 0 && kind < kKinds, "sgrender: export_image: unknown kind ", kind, " (0 albedo, 1 normal, 2 rough, 3 depth, 4 rendered, 5 shading, 6 image, 7 image_gamma)");
  const char* name = kKindNames[kind];
  TORCH_CHECK(x.scalar_type() == at::kFloat, "sgrender: export_image(", name, "): x must be fp32, got ", x.scalar_type());
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0, "sgrender: export_image(", name, "): x must be a non-empty [B,C,h,w], got ", x.sizes());
  TORCH_CHECK(kind_takes(kind, x.size(1)), "sgrender: export_image(", name, "): this kind takes C = ", kind_channels(kind), ", got x ", x.sizes());
  int64_t nh = x.size(2), nw = x.size(3);
  if (size.has_value()) {
    TORCH_CHECK(size->size() == 2 && (*size)[0] > 0 && (*size)[1] > 0, "sgrender: export_image(", name, "): size must be two positive integers (nh, nw), got ", *size);
    nh = (*size)[0];
    nw = (*size)[1];
    TORCH_CHECK(kind_resizes(kind) || (nh == x.size(2) && nw == x.size(3)), "sgrender: export_image(", name, "): this kind is written at the source's size ", x.size(2), " x ",
                x.size(3), " (the reference does not resize it), got size ", *size);
  }
  if (has(scale)) {
    TORCH_CHECK(kind == SGR_EXPORT_ALBEDO, "sgrender: export_image(", name, "): scale (cAlbedo) belongs to the albedo kind");
    if (device) TORCH_CHECK(scale->is_cuda(), kNoCpu);
    TORCH_CHECK(scale->device() == x.device(), "sgrender: export_image: tensors on different devices (", x.device(), " vs ", scale->device(), ")");
    TORCH_CHECK(scale->scalar_type() == at::kFloat, "sgrender: export_image(albedo): scale must be fp32, got ", scale->scalar_type());
    TORCH_CHECK(scale->numel() == x.size(0), "sgrender: export_image(albedo): scale must hold one value per image (", x.size(0), "), got ", scale->sizes());
  }
  TORCH_CHECK(x.size(0) <= 65535 && x.size(1) * x.size(2) * x.size(3) < (int64_t(1) << 30) && nh * nw < (int64_t(1) << 30) && nh <= 1048560, "sgrender: export_image(", name,
              "): x ", x.sizes(), " -> ", nh, " x ", nw, " is out of range (B <= 65535, C h w < 2^30, nh nw < 2^30)");
  return {nh, nw};
}
Tensor image_alloc(const Tensor& x, int64_t kind, int64_t nh, int64_t nw) { return at::empty({x.size(0), nh, nw, kind >= SGR_EXPORT_IMAGE ? 3 : x.size(1)}, u8(x)); }
Tensor export_image_cuda(const Tensor& x, int64_t kind, at::OptionalIntArrayRef size, const OptTensor& scale, bool bgr) {
  const auto [nh, nw] = image_check(x, kind, size, scale, true);
  const c10::DeviceGuard guard(x.device());
  const Tensor s = has(scale) ? scale->contiguous() : Tensor();
  Tensor out = image_alloc(x, kind, nh, nw);
  const long long need = api().sgr_export_image_workspace_floats((int)kind, (int)x.size(0));
  const Tensor ws = need > 0 ? at::empty({(int64_t)need}, x.options().memory_format(at::MemoryFormat::Contiguous)) : Tensor();
  const Strides4 st = strides_of(x);
  ok(api().sgr_export_image(rp(x), st.v, rp(s), bwp(out), wp(ws), (int)kind, (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)nh, (int)nw, bgr,
                            stream_of(x.device())),
     "sgr_export_image");
  return out;
}
Tensor export_image_meta(const Tensor& x, int64_t kind, at::OptionalIntArrayRef size, const OptTensor& scale, bool) {
  const auto [nh, nw] = image_check(x, kind, size, scale, false);
  return image_alloc(x, kind, nh, nw);
}

// ---- env images -------------------------------------------------------------------------------------------------------------------------
void env_check(const Tensor& env, const char* op, bool device) {
  if (device) TORCH_CHECK(env.is_cuda(), kNoCpu);
  TORCH_CHECK(env.scalar_type() == at::kFloat, "sgrender: ", op, ": env must be fp32, got ", env.scalar_type());
  TORCH_CHECK(env.dim() == 6 && env.size(1) == 3 && env.numel() > 0, "sgrender: ", op, ": env must be a non-empty [B,3,R,C,eh,ew], got ", env.sizes());
}
// -> (Hm, Wm)
std::pair<int64_t, int64_t> mosaic_check(const Tensor& env, int64_t nrows, int64_t ncols, int64_t gap, bool device) {
  env_check(env, "export_env_mosaic", device);
  const int64_t R = env.size(2), C = env.size(3), eh = env.size(4), ew = env.size(5);
  TORCH_CHECK(nrows > 0 && ncols > 0 && gap >= 0, "sgrender: export_env_mosaic: nrows and ncols must be positive and gap not negative, got ", nrows, ", ", ncols, ", ", gap);
  TORCH_CHECK(nrows <= R && ncols <= C, "sgrender: export_env_mosaic: nrows = ", nrows, ", ncols = ", ncols, " exceed the grid ", R, " x ", C,
              " (int(R / nrows) would be 0: utils.writeEnvToFile divides by zero there)");
  const int64_t interY = R / nrows, interX = C / ncols;
  const int64_t Hm = (R + interY - 1) / interY * (eh + gap) + gap, Wm = (C + interX - 1) / interX * (ew + gap) + gap;
  TORCH_CHECK(env.size(0) <= 65535 && Hm <= 65535 && Hm * Wm < (int64_t(1) << 29), "sgrender: export_env_mosaic: env ", env.sizes(), " -> ", Hm, " x ", Wm,
              " is out of range (B, Hm <= 65535, Hm Wm < 2^29)");
  return {Hm, Wm};
}
Tensor export_env_mosaic_cuda(const Tensor& env, int64_t nrows, int64_t ncols, int64_t gap, bool bgr) {
  const auto [Hm, Wm] = mosaic_check(env, nrows, ncols, gap, true);
  const c10::DeviceGuard guard(env.device());
  Tensor out = at::empty({env.size(0), Hm, Wm, 3}, u8(env));
  long long st[6];
  for (int i = 0; i < 6; ++i) st[i] = (long long)env.stride(i);
  ok(api().sgr_export_env_mosaic(rp(env), st, bwp(out), (int)env.size(0), (int)env.size(2), (int)env.size(3), (int)env.size(4), (int)env.size(5), (int)nrows, (int)ncols, (int)gap,
                                 bgr, stream_of(env.device())),
     "sgr_export_env_mosaic");
  return out;
}
Tensor export_env_mosaic_meta(const Tensor& env, int64_t nrows, int64_t ncols, int64_t gap, bool) {
  const auto [Hm, Wm] = mosaic_check(env, nrows, ncols, gap, false);
  return at::empty({env.size(0), Hm, Wm, 3}, u8(env));
}

Tensor hwc_alloc(const Tensor& env) {
  return at::empty({env.size(0), env.size(2), env.size(3), env.size(4), env.size(5), 3}, env.options().memory_format(at::MemoryFormat::Contiguous));
}
Tensor export_env_hwc_cuda(const Tensor& env, bool flip) {
  env_check(env, "export_env_hwc", true);
  TORCH_CHECK(env.size(2) * env.size(3) < (int64_t(1) << 31) && env.size(4) * env.size(5) < (int64_t(1) << 28), "sgrender: export_env_hwc: env ", env.sizes(),
              " is out of range (R C < 2^31, eh ew < 2^28)");
  const c10::DeviceGuard guard(env.device());
  const Tensor e = env.contiguous();      // a view is copied once; the kernel picks its 128-bit path by the pointers' alignment
  Tensor out = hwc_alloc(e);
  ok(api().sgr_export_env_hwc(rp(e), wp(out), (int)e.size(0), (int)e.size(2), (int)e.size(3), (int)e.size(4), (int)e.size(5), flip, stream_of(env.device())), "sgr_export_env_hwc");
  return out;
}
Tensor export_env_hwc_meta(const Tensor& env, bool) {
  env_check(env, "export_env_hwc", false);
  return hwc_alloc(env);
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("export_image(Tensor x, int kind, int[]? size=None, Tensor? scale=None, bool bgr=False) -> Tensor");
  m.def("export_env_mosaic(Tensor env, int nrows=12, int ncols=8, int gap=1, bool bgr=False) -> Tensor");
  m.def("export_env_hwc(Tensor env, bool flip=True) -> Tensor");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("export_image", &export_image_cuda);
  m.impl("export_env_mosaic", &export_env_mosaic_cuda);
  m.impl("export_env_hwc", &export_env_hwc_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("export_image", &export_image_meta);
  m.impl("export_env_mosaic", &export_env_mosaic_meta);
  m.impl("export_env_hwc", &export_env_hwc_meta);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"export_image", "export_env_mosaic", "export_env_hwc"}); }

// torch.ops.sgrender.pil_resize: PIL's antialiased resize of 8-bit images (dataLoader.py:223-224, iiwDataLoader.py:112-134) as an operator of
// the C++ torch extension.
//
// Same rules as sgr_torch.cpp: the operator checks its arguments -- one check_pil_resize shared by the device and the Meta kernel, so that a
// traced graph cannot pass tracing and then fail on the device --, allocates the output and the workspace with the caching allocator and calls
// the C ABI (sgr_pil_resize_u8 of include/sgrender.h) on the current HIP stream.  The coefficient tables are built on the host ONCE per
// (inSize, outSize, filter, device) and kept on the device: the first call of a geometry copies them there, every later one is a lookup, does
// no host-device traffic and so captures in a HIP graph.  Bytes in, bytes out: no autograd node.
#include <map>
#include <mutex>
#include <vector>

#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

constexpr const char* kPilHost = "; on the host it is PIL's Image.resize(size, Image.LANCZOS) (Image.ANTIALIAS in the reference) of the decoded image";

// PIL's codes (Image.Resampling)
int filter_code(c10::string_view name) {
  if (name == "lanczos" || name == "antialias") return 1;
  if (name == "bilinear") return 2;
  if (name == "bicubic") return 3;
  if (name == "box") return 4;
  if (name == "hamming") return 5;
  TORCH_CHECK(name != "nearest", "sgrender: pil_resize: filter 'nearest' is a different PIL code path (no coefficients, no antialiasing): not offered; index the tensor instead");
  TORCH_CHECK(false, "sgrender: pil_resize: unknown filter '", name, "' (lanczos -- the reference's ANTIALIAS --, bilinear, bicubic, box or hamming)");
  return 0;
}
int path_code(c10::string_view name) {
  if (name == "auto") return SGR_PIL_RESIZE_AUTO;
  if (name == "two_pass") return SGR_PIL_RESIZE_TWO_PASS;
  if (name == "tiled") return SGR_PIL_RESIZE_TILED;
  TORCH_CHECK(false, "sgrender: pil_resize: unknown path '", name, "' (auto, two_pass or tiled)");
  return 0;
}

struct PilDims { int64_t bn, H, W, C, r0, c0, h, w; int filter, path; bool batched, windowed; };

PilDims check_pil_resize(const Tensor& im, int64_t width, int64_t height, c10::string_view filter, at::OptionalIntArrayRef window, c10::string_view path, bool device) {
  if (device) TORCH_CHECK(im.is_cuda(), kNoCpu);
  TORCH_CHECK(im.scalar_type() == at::kByte, "sgrender: pil_resize: im_u8 must be uint8 (the decoded file), got ", im.scalar_type(),
              " (PIL resamples float and 32-bit integer images on another route, which is not offered)", kPilHost);
  TORCH_CHECK(im.dim() == 3 || im.dim() == 4, "sgrender: pil_resize: im_u8 must be [H,W,C] or [bn,H,W,C] (the layout the file readers hand over), got ", im.sizes());
  PilDims d{};
  d.batched = im.dim() == 4;
  const int o = d.batched ? 1 : 0;
  d.bn = d.batched ? im.size(0) : 1;
  d.H = im.size(o);
  d.W = im.size(o + 1);
  d.C = im.size(o + 2);
  TORCH_CHECK(d.C == 1 || d.C == 3, "sgrender: pil_resize: C must be 1 ('L') or 3 ('RGB'), got ", d.C,
              ": PIL resizes LA / RGBA on its premultiplied-alpha route, which is not offered", kPilHost);
  TORCH_CHECK(im.numel() > 0, "sgrender: pil_resize: zero-sized input ", im.sizes());
  TORCH_CHECK(width > 0 && height > 0, "sgrender: pil_resize: zero-sized or negative output size (width, height) = (", width, ", ", height, ")");
  d.filter = filter_code(filter);
  d.path = path_code(path);
  constexpr int64_t kSide = int64_t(1) << 24, kImage = int64_t(1) << 31;
  TORCH_CHECK(d.bn <= 65535 && d.H <= kSide && d.W <= kSide && width <= kSide && height <= kSide && d.H * d.W * d.C < kImage && width * height * d.C < kImage,
              "sgrender: pil_resize: ", im.sizes(), " -> (", width, ", ", height, ") is out of range (bn <= 65535, every side <= 2^24, H W C < 2^31)", kPilHost);
  d.r0 = 0;
  d.c0 = 0;
  d.h = height;
  d.w = width;
  d.windowed = window.has_value();
  if (d.windowed) {
    TORCH_CHECK(window->size() == 4, "sgrender: pil_resize: window must be (r0, c0, h, w), got ", window->size(), " values");
    d.r0 = (*window)[0];
    d.c0 = (*window)[1];
    d.h = (*window)[2];
    d.w = (*window)[3];
    TORCH_CHECK(d.h > 0 && d.w > 0, "sgrender: pil_resize: window (r0, c0, h, w) = ", *window, " is zero-sized");
    TORCH_CHECK(d.r0 >= 0 && d.c0 >= 0 && d.r0 + d.h <= height && d.c0 + d.w <= width, "sgrender: pil_resize: window (r0, c0, h, w) = ", *window, " leaves the resized image ", height,
                " x ", width);
  }
  return d;
}
Tensor pil_alloc(const Tensor& im, const PilDims& d) {
  const auto o = im.options().memory_format(at::MemoryFormat::Contiguous);
  return d.batched ? at::empty({d.bn, d.h, d.w, d.C}, o) : at::empty({d.h, d.w, d.C}, o);
}

// (inSize, outSize, filter, device index) -> the table on that device
const Tensor& device_table(int in, int out, int filter, const c10::Device& dev) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int>, Tensor> cache;
  const std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(in, out, filter, (int)dev.index());
  auto it = cache.find(key);
  if (it == cache.end()) {
    const long long n = api().sgr_pil_resize_table_ints(in, out, filter);
    TORCH_CHECK(n > 0, "sgrender: sgr_pil_resize_table_ints failed (code ", n, "): ", api().sgr_last_error());
    std::vector<int> host((size_t)n);
    ok(api().sgr_pil_resize_table(in, out, filter, host.data()), "sgr_pil_resize_table");
    const Tensor t = at::from_blob(host.data(), {(int64_t)n}, at::TensorOptions().dtype(at::kInt)).to(dev);      // a synchronous copy: `host` may go
    it = cache.emplace(key, t).first;
  }
  return it->second;
}

Tensor pil_resize_cuda(const Tensor& im, int64_t width, int64_t height, c10::string_view filter, at::OptionalIntArrayRef window, c10::string_view path) {
  const PilDims d = check_pil_resize(im, width, height, filter, window, path, true);
  const c10::DeviceGuard guard(im.device());
  const Tensor src = im.contiguous();
  Tensor out = pil_alloc(src, d);
  const int win[4] = {(int)d.r0, (int)d.c0, (int)d.h, (int)d.w};
  const int* wp4 = d.windowed ? win : nullptr;
  const int* ht = width != d.W ? device_table((int)d.W, (int)width, d.filter, im.device()).const_data_ptr<int>() : nullptr;
  const int* vt = height != d.H ? device_table((int)d.H, (int)height, d.filter, im.device()).const_data_ptr<int>() : nullptr;
  const long long bytes = api().sgr_pil_resize_workspace_bytes((int)d.bn, (int)d.H, (int)d.W, (int)d.C, (int)height, (int)width, wp4, d.filter);
  TORCH_CHECK(bytes >= 0, "sgrender: sgr_pil_resize_workspace_bytes failed (code ", bytes, "): ", api().sgr_last_error());
  Tensor ws;      // the two_pass route's intermediate; none where the call goes tiled
  const bool tiled = d.path == SGR_PIL_RESIZE_TILED ||
                     (d.path == SGR_PIL_RESIZE_AUTO && api().sgr_pil_resize_route((int)d.bn, (int)d.H, (int)d.W, (int)d.C, (int)height, (int)width, wp4, d.filter) == SGR_PIL_RESIZE_TILED);
  if (bytes > 0 && !tiled) ws = at::empty({(int64_t)bytes}, src.options());
  ok(api().sgr_pil_resize_u8(src.const_data_ptr<uint8_t>(), (int)d.bn, (int)d.H, (int)d.W, (int)d.C, out.data_ptr<uint8_t>(), (int)height, (int)width, wp4, d.filter, ht, vt,
                             ws.defined() ? ws.data_ptr<uint8_t>() : nullptr, d.path, stream_of(im.device())),
     "sgr_pil_resize_u8");
  return out;
}
Tensor pil_resize_meta(const Tensor& im, int64_t width, int64_t height, c10::string_view filter, at::OptionalIntArrayRef window, c10::string_view path) {
  return pil_alloc(im, check_pil_resize(im, width, height, filter, window, path, false));
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("pil_resize(Tensor im_u8, int width, int height, str filter=\"lanczos\", int[]? window=None, str path=\"auto\") -> Tensor");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) { m.impl("pil_resize", &pil_resize_cuda); }
TORCH_LIBRARY_IMPL(sgrender, Meta, m) { m.impl("pil_resize", &pil_resize_meta); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"pil_resize"}); }

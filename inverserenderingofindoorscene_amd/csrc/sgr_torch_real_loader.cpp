// torch.ops.sgrender.nyu_prepare / iiw_image: the real-image loaders' batch preparation (nyuDataLoader.py:75-131, iiwDataLoader.py:136-137,
// 205-214) as operators of the C++ torch extension.
//
// Same rules as sgr_torch.cpp: an operator checks its arguments -- one check shared by the device and the Meta kernel, so that a traced graph
// cannot pass tracing and then fail on the device --, allocates the outputs with the caching allocator and calls the C ABI (sgr_nyu_prepare,
// sgr_iiw_image of include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.  The results are inputs of
// the training step: no autograd node.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

constexpr const char* kNyuNumpy = "; on the host it is nyuDataLoader.py's crop, loadImage, cv2.resize(INTER_LINEAR) and the two normalisations";
constexpr const char* kIiwNumpy = "; on the host it is (im / 255.0) ** 2.2, np.transpose(im, [2, 0, 1]) and im / im.max()";

const unsigned char* bp(const Tensor& t) { return t.const_data_ptr<uint8_t>(); }
at::TensorOptions f32(const Tensor& like) { return like.options().dtype(at::kFloat).memory_format(at::MemoryFormat::Contiguous); }

// a non-empty uint8 [bn,H,W,3]
void check_u8_hwc3(const Tensor& t, const char* op, const char* name, const char* numpy, bool device) {
  if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
  TORCH_CHECK(t.scalar_type() == at::kByte, "sgrender: ", op, ": ", name, " must be uint8 (the decoded file), got ", t.scalar_type(), numpy);
  TORCH_CHECK(t.dim() == 4 && t.size(3) == 3 && t.numel() > 0, "sgrender: ", op, ": ", name, " must be a non-empty [bn,H,W,3] (the layout the file readers hand over), got ",
              t.sizes(), numpy);
  TORCH_CHECK(t.size(0) <= 65535 && t.size(1) * t.size(2) < (int64_t(1) << 28), "sgrender: ", op, ": ", name, " ", t.sizes(), " is out of range (bn <= 65535, H W < 2^28)", numpy);
}

// ---- nyu_prepare ------------------------------------------------------------------------------------------------------------------------
void per_image(const Tensor& t, const Tensor& ref, at::ScalarType type, std::initializer_list<int64_t> shape, const char* name, const char* what, bool device) {
  if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
  TORCH_CHECK(t.device() == ref.device(), "sgrender: nyu_prepare: tensors on different devices (", ref.device(), " vs ", t.device(), ")");
  TORCH_CHECK(t.scalar_type() == type, "sgrender: nyu_prepare: ", name, " must be ", type, " (", what, "), got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == at::IntArrayRef(shape), "sgrender: nyu_prepare: ", name, " must be ", at::IntArrayRef(shape), " (mismatched batch sizes?), got ", t.sizes());
}
void nyu_check(const Tensor& im, const Tensor& normal, const Tensor& seg, const Tensor& depth, const OptTensor& crop, const OptTensor& flip, const OptTensor& colour, int64_t H,
               int64_t W, bool device) {
  check_u8_hwc3(im, "nyu_prepare", "im_u8", kNyuNumpy, device);
  check_u8_hwc3(normal, "nyu_prepare", "normal_u8", kNyuNumpy, device);
  check_u8_hwc3(seg, "nyu_prepare", "seg_u8", kNyuNumpy, device);
  if (device) TORCH_CHECK(depth.is_cuda(), kNoCpu);
  TORCH_CHECK(depth.scalar_type() == at::kFloat, "sgrender: nyu_prepare: depth must be fp32, got ", depth.scalar_type(),
              " (a uint16 TIFF is not what the reference's loader reads: convert it on the host to the fp32 depth the files hold)");
  TORCH_CHECK(depth.dim() == 3, "sgrender: nyu_prepare: depth must be [bn,Hs,Ws], got ", depth.sizes());
  for (const Tensor* t : {&normal, &seg}) {
    TORCH_CHECK(t->device() == im.device(), "sgrender: nyu_prepare: tensors on different devices (", im.device(), " vs ", t->device(), ")");
    TORCH_CHECK(t->sizes() == im.sizes(), "sgrender: nyu_prepare: im_u8 ", im.sizes(), ", normal_u8 ", normal.sizes(), " and seg_u8 ", seg.sizes(),
                " must share [bn,Hs,Ws,3] (mismatched batch sizes?)");
  }
  TORCH_CHECK(depth.device() == im.device(), "sgrender: nyu_prepare: tensors on different devices (", im.device(), " vs ", depth.device(), ")");
  TORCH_CHECK(depth.size(0) == im.size(0) && depth.size(1) == im.size(1) && depth.size(2) == im.size(2), "sgrender: nyu_prepare: depth ", depth.sizes(), " and im_u8 ", im.sizes(),
              " must share [bn,Hs,Ws] (mismatched batch sizes?)");
  TORCH_CHECK(H > 0 && W > 0, "sgrender: nyu_prepare: imHeight and imWidth must be positive, got ", H, " x ", W);
  TORCH_CHECK(H * W < (int64_t(1) << 28) && H <= 1048560, "sgrender: nyu_prepare: imHeight x imWidth = ", H, " x ", W, " is out of range (H W < 2^28)", kNyuNumpy);
  TORCH_CHECK(has(crop) == has(flip) && has(crop) == has(colour), "sgrender: nyu_prepare: crop, flip and colour come all three (the TRAIN phase) or not at all (TEST)");
  if (has(crop)) {
    const int64_t bn = im.size(0);
    per_image(*crop, im, at::kInt, {bn, 4}, "crop", "(rs, cs, cropH, cropW) per image", device);
    per_image(*flip, im, at::kBool, {bn}, "flip", "one flag per image", device);
    per_image(*colour, im, at::kDouble, {bn, 3}, "colour", "numpy's float64 scale", device);
  }
}
T5 nyu_alloc(const Tensor& im, int64_t H, int64_t W) {
  const auto o = f32(im);
  const int64_t bn = im.size(0);
  return {at::empty({bn, 3, H, W}, o), at::empty({bn, 1, H, W}, o), at::empty({bn, 1, H, W}, o), at::empty({bn, 1, H, W}, o), at::empty({bn, 3, H, W}, o)};
}
// -> (normal, depth, segNormal, segDepth, im)
T5 nyu_prepare_cuda(const Tensor& im, const Tensor& normal, const Tensor& seg, const Tensor& depth, const OptTensor& crop, const OptTensor& flip, const OptTensor& colour, int64_t H,
                    int64_t W) {
  nyu_check(im, normal, seg, depth, crop, flip, colour, H, W, true);
  const c10::DeviceGuard guard(im.device());
  const Tensor i = im.contiguous(), n = normal.contiguous(), s = seg.contiguous(), d = depth.contiguous();
  const bool train = has(crop);
  const Tensor c = train ? crop->contiguous() : Tensor(), f = train ? flip->contiguous() : Tensor(), k = train ? colour->contiguous() : Tensor();
  T5 out = nyu_alloc(i, H, W);
  ok(api().sgr_nyu_prepare(bp(i), bp(n), bp(s), rp(d), train ? c.const_data_ptr<int>() : nullptr, train ? reinterpret_cast<const unsigned char*>(f.const_data_ptr<bool>()) : nullptr,
                           train ? k.const_data_ptr<double>() : nullptr, wp(std::get<0>(out)), wp(std::get<1>(out)), wp(std::get<2>(out)), wp(std::get<3>(out)), wp(std::get<4>(out)),
                           (int)i.size(0), (int)i.size(1), (int)i.size(2), (int)H, (int)W, stream_of(im.device())),
     "sgr_nyu_prepare");
  return out;
}
T5 nyu_prepare_meta(const Tensor& im, const Tensor& normal, const Tensor& seg, const Tensor& depth, const OptTensor& crop, const OptTensor& flip, const OptTensor& colour, int64_t H,
                    int64_t W) {
  nyu_check(im, normal, seg, depth, crop, flip, colour, H, W, false);
  return nyu_alloc(im, H, W);
}

// ---- iiw_image --------------------------------------------------------------------------------------------------------------------------
Tensor iiw_image_cuda(const Tensor& im) {
  check_u8_hwc3(im, "iiw_image", "im_u8", kIiwNumpy, true);
  const c10::DeviceGuard guard(im.device());
  const Tensor i = im.contiguous();
  Tensor out = at::empty({i.size(0), 3, i.size(1), i.size(2)}, f32(i));
  const Tensor ws = at::empty({64 * i.size(0)}, f32(i));
  ok(api().sgr_iiw_image(bp(i), wp(out), wp(ws), (int)i.size(0), (int)i.size(1), (int)i.size(2), stream_of(im.device())), "sgr_iiw_image");
  return out;
}
Tensor iiw_image_meta(const Tensor& im) {
  check_u8_hwc3(im, "iiw_image", "im_u8", kIiwNumpy, false);
  return at::empty({im.size(0), 3, im.size(1), im.size(2)}, f32(im));
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("nyu_prepare(Tensor im_u8, Tensor normal_u8, Tensor seg_u8, Tensor depth, Tensor? crop, Tensor? flip, Tensor? colour, int imHeight=480, int imWidth=640) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("iiw_image(Tensor im_u8) -> Tensor");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("nyu_prepare", &nyu_prepare_cuda);
  m.impl("iiw_image", &iiw_image_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("nyu_prepare", &nyu_prepare_meta);
  m.impl("iiw_image", &iiw_image_meta);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"nyu_prepare", "iiw_image"}); }

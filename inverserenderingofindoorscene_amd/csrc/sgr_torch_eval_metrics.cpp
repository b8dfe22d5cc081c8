// torch.ops.sgrender.eval_*: the reference's three evaluation metrics (CompareWHDR.py:8-66, CompareNormal.py:18-42, CompareDepth.py:16-32) as
// operators of the C++ torch extension.
//
// Same rules as sgr_torch.cpp: an operator checks its arguments -- one check shared by the device and the Meta kernel, so that a traced graph
// cannot pass tracing and then fail on the device --, allocates the outputs with the caching allocator and calls the C ABI (sgr_eval_* of
// include/sgrender.h) on the current HIP stream; nothing here computes and nothing synchronises.  The fp32 maps travel with their strides
// (channels-last maps and slices are not copied); the byte images and the judgement arrays are made contiguous.  Metrics: no autograd node.
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

constexpr int64_t kRange = int64_t(1) << 28;

at::TensorOptions opt(const Tensor& like, at::ScalarType t) { return like.options().dtype(t).memory_format(at::MemoryFormat::Contiguous); }
bool is_int(const Tensor& t) { return t.scalar_type() == at::kInt || t.scalar_type() == at::kLong; }
void same_device(const Tensor& t, const Tensor& ref, const char* op, bool device) {
  if (device) TORCH_CHECK(t.is_cuda(), kNoCpu);
  TORCH_CHECK(t.device() == ref.device(), "sgrender: ", op, ": tensors on different devices (", ref.device(), " vs ", t.device(), ")");
}

// ---- whdr ---------------------------------------------------------------------------------------------------------------------------------
struct WhdrDims { int64_t B, H, W, N; bool u8; };
WhdrDims whdr_check(const Tensor& r, const Tensor& point, const Tensor& weight, const Tensor& label, const Tensor& num, double delta, bool device) {
  if (device) TORCH_CHECK(r.is_cuda(), kNoCpu);
  const bool u8 = r.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || r.scalar_type() == at::kFloat, "sgrender: whdr: reflectance must be fp32 [B,3,H,W] or uint8 [B,H,W,3] (the saved PNG), got ", r.scalar_type());
  TORCH_CHECK(r.dim() == 4 && r.numel() > 0 && r.size(u8 ? 3 : 1) == 3, "sgrender: whdr: reflectance must be a non-empty ", u8 ? "uint8 [B,H,W,3]" : "fp32 [B,3,H,W]", ", got ",
              r.sizes());
  const int64_t B = r.size(0), H = r.size(u8 ? 1 : 2), W = r.size(u8 ? 2 : 3);
  for (const Tensor* t : {&point, &weight, &label, &num}) same_device(*t, r, "whdr", device);
  TORCH_CHECK(point.dim() == 3 && point.size(0) == B && point.size(2) == 4 && point.size(1) > 0, "sgrender: whdr: point must be [", B, ",N,4] = (r1, c1, r2, c2) with N > 0, got ",
              point.sizes());
  TORCH_CHECK(is_int(point), "sgrender: whdr: point must be int32 or int64, got ", point.scalar_type());
  const int64_t N = point.size(1);
  TORCH_CHECK(weight.scalar_type() == at::kFloat, "sgrender: whdr: weight must be fp32, got ", weight.scalar_type());
  TORCH_CHECK(weight.sizes() == at::IntArrayRef({B, N}), "sgrender: whdr: weight must be [", B, ",", N, "] (point's B and N), got ", weight.sizes());
  TORCH_CHECK(at::isIntegralType(label.scalar_type(), false), "sgrender: whdr: label must be an integer tensor (0 'E', 1 '1', 2 '2'), got ", label.scalar_type());
  TORCH_CHECK(label.sizes() == at::IntArrayRef({B, N}), "sgrender: whdr: label must be [", B, ",", N, "] (point's B and N), got ", label.sizes());
  TORCH_CHECK(is_int(num) && num.dim() == 1 && num.size(0) == B, "sgrender: whdr: num must be int32 or int64 [", B, "], got ", num.scalar_type(), " ", num.sizes());
  TORCH_CHECK(delta >= 0.0, "sgrender: whdr: delta must not be negative, got ", delta);
  TORCH_CHECK(B <= 65535 && H * W < kRange && N < kRange, "sgrender: whdr: reflectance ", r.sizes(), " with N = ", N, " is out of range (B <= 65535, H W < 2^28, N < 2^28)");
  return {B, H, W, N, u8};
}
T4 whdr_alloc(const Tensor& r, int64_t B) { return {at::empty({B}, opt(r, at::kFloat)), at::empty({B}, opt(r, at::kFloat)), at::empty({B}, opt(r, at::kFloat)), at::empty({B, 6}, opt(r, at::kDouble))}; }
// -> (whdr, equal, inequal, sums)
T4 eval_whdr_cuda(const Tensor& r, const Tensor& point, const Tensor& weight, const Tensor& label, const Tensor& num, double delta) {
  const WhdrDims d = whdr_check(r, point, weight, label, num, delta, true);
  const c10::DeviceGuard guard(r.device());
  const Tensor p = point.to(at::kInt).contiguous(), w = weight.contiguous(), l = label.to(at::kInt).contiguous(), n = num.to(at::kInt).contiguous();
  const Tensor out3 = at::empty({3, d.B}, opt(r, at::kFloat)), sums = at::empty({d.B, 6}, opt(r, at::kDouble));
  const long long st[4] = {(long long)r.stride(0), (long long)r.stride(d.u8 ? 3 : 1), (long long)r.stride(d.u8 ? 1 : 2), (long long)r.stride(d.u8 ? 2 : 3)};
  ok(api().sgr_eval_whdr(r.const_data_ptr(), st, d.u8 ? 1 : 0, p.const_data_ptr<int>(), rp(w), l.const_data_ptr<int>(), n.const_data_ptr<int>(), sums.data_ptr<double>(), wp(out3),
                         (int)d.B, (int)d.H, (int)d.W, (int)d.N, (float)delta, stream_of(r.device())),
     "sgr_eval_whdr");
  return {out3[0], out3[1], out3[2], sums};
}
T4 eval_whdr_meta(const Tensor& r, const Tensor& point, const Tensor& weight, const Tensor& label, const Tensor& num, double delta) {
  return whdr_alloc(r, whdr_check(r, point, weight, label, num, delta, false).B);
}

// ---- normal angle -------------------------------------------------------------------------------------------------------------------------
void normal_check(const Tensor& pred, const Tensor& gt, const Tensor& mask, bool device) {
  if (device) TORCH_CHECK(pred.is_cuda(), kNoCpu);
  TORCH_CHECK(pred.scalar_type() == at::kFloat, "sgrender: normal_angle_error: normalPred must be fp32, got ", pred.scalar_type());
  TORCH_CHECK(pred.dim() == 4 && pred.size(1) == 3 && pred.numel() > 0, "sgrender: normal_angle_error: normalPred must be a non-empty [B,3,h,w], got ", pred.sizes());
  same_device(gt, pred, "normal_angle_error", device);
  same_device(mask, pred, "normal_angle_error", device);
  TORCH_CHECK(gt.scalar_type() == at::kByte && mask.scalar_type() == at::kByte, "sgrender: normal_angle_error: normalGt and mask must be uint8 (the decoded PNGs), got ",
              gt.scalar_type(), " and ", mask.scalar_type());
  TORCH_CHECK(gt.dim() == 4 && gt.size(3) == 3 && gt.size(0) == pred.size(0) && gt.numel() > 0, "sgrender: normal_angle_error: normalGt must be a non-empty [", pred.size(0),
              ",H,W,3] in RGB order, got ", gt.sizes());
  const bool m3 = mask.dim() == 4 && mask.size(3) == 3, m1 = mask.dim() == 3;
  TORCH_CHECK((m3 || m1) && mask.size(0) == gt.size(0) && mask.size(1) == gt.size(1) && mask.size(2) == gt.size(2), "sgrender: normal_angle_error: mask must be [B,H,W,3] or [B,H,W] of normalGt's ",
              gt.sizes(), ", got ", mask.sizes());
  TORCH_CHECK(pred.size(0) <= 65535 && pred.size(2) * pred.size(3) < kRange && gt.size(1) * gt.size(2) < kRange, "sgrender: normal_angle_error: ", pred.sizes(), " -> ", gt.sizes(),
              " is out of range (B <= 65535, h w < 2^28, H W < 2^28)");
}
T4 normal_alloc(const Tensor& pred, const Tensor& gt) {
  const int64_t B = gt.size(0);
  return {at::empty({B}, opt(pred, at::kFloat)), at::empty({B}, opt(pred, at::kFloat)), at::empty({B}, opt(pred, at::kInt)), at::empty({B, gt.size(1), gt.size(2)}, opt(pred, at::kFloat))};
}
// -> (mean, median, count, theta)
T4 eval_normal_angle_cuda(const Tensor& pred, const Tensor& gt, const Tensor& mask) {
  normal_check(pred, gt, mask, true);
  const c10::DeviceGuard guard(pred.device());
  const Tensor g = gt.contiguous(), m = mask.contiguous();
  const int64_t B = g.size(0), H = g.size(1), W = g.size(2);
  T4 out = normal_alloc(pred, g);
  const Tensor keys = at::empty({B, H, W}, opt(pred, at::kInt));
  const Tensor partials = at::empty({(int64_t)api().sgr_eval_partials_doubles((int)B, 3)}, opt(pred, at::kDouble));
  const Strides4 st = strides_of(pred);
  ok(api().sgr_eval_normal_angle(rp(pred), st.v, g.const_data_ptr<uint8_t>(), m.const_data_ptr<uint8_t>(), m.dim() == 4 ? 3 : 1, wp(std::get<3>(out)),
                                 reinterpret_cast<unsigned*>(keys.data_ptr<int>()), partials.data_ptr<double>(), wp(std::get<0>(out)), wp(std::get<1>(out)),
                                 std::get<2>(out).data_ptr<int>(), (int)B, (int)pred.size(2), (int)pred.size(3), (int)H, (int)W, stream_of(pred.device())),
     "sgr_eval_normal_angle");
  return out;
}
T4 eval_normal_angle_meta(const Tensor& pred, const Tensor& gt, const Tensor& mask) {
  normal_check(pred, gt, mask, false);
  return normal_alloc(pred, gt);
}

// ---- log-depth RMSE -----------------------------------------------------------------------------------------------------------------------
// [B,h,w], or [B,1,h,w] seen as it
Tensor plane(const Tensor& t, const char* name, const char* shape) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, "sgrender: depth_log_rmse: ", name, " must be fp32, got ", t.scalar_type());
  TORCH_CHECK((t.dim() == 3 || (t.dim() == 4 && t.size(1) == 1)) && t.numel() > 0, "sgrender: depth_log_rmse: ", name, " must be a non-empty ", shape, ", got ", t.sizes());
  return t.dim() == 4 ? t.select(1, 0) : t;
}
T2 depth_views(const Tensor& pred, const Tensor& gt, bool device) {
  if (device) TORCH_CHECK(pred.is_cuda(), kNoCpu);
  same_device(gt, pred, "depth_log_rmse", device);
  const Tensor p = plane(pred, "depthPred", "[B,1,h,w] or [B,h,w]"), g = plane(gt, "depthGt", "[B,H,W] or [B,1,H,W]");
  TORCH_CHECK(p.size(0) == g.size(0), "sgrender: depth_log_rmse: depthPred ", pred.sizes(), " and depthGt ", gt.sizes(), " must share B (mismatched batch sizes?)");
  TORCH_CHECK(p.size(0) <= 65535 && p.size(1) * p.size(2) < kRange && g.size(1) * g.size(2) < kRange, "sgrender: depth_log_rmse: ", pred.sizes(), " -> ", gt.sizes(),
              " is out of range (B <= 65535, h w < 2^28, H W < 2^28)");
  return {p, g};
}
T2 depth_alloc(const Tensor& p) { return {at::empty({p.size(0)}, opt(p, at::kFloat)), at::empty({p.size(0)}, opt(p, at::kInt))}; }
// -> (rmse, count)
T2 eval_depth_log_rmse_cuda(const Tensor& pred, const Tensor& gt) {
  const auto [p, g] = depth_views(pred, gt, true);
  const c10::DeviceGuard guard(pred.device());
  T2 out = depth_alloc(p);
  const Tensor partials = at::empty({(int64_t)api().sgr_eval_partials_doubles((int)p.size(0), 5)}, opt(p, at::kDouble));
  const long long ps[3] = {(long long)p.stride(0), (long long)p.stride(1), (long long)p.stride(2)}, gs[3] = {(long long)g.stride(0), (long long)g.stride(1), (long long)g.stride(2)};
  ok(api().sgr_eval_depth_log_rmse(rp(p), ps, rp(g), gs, partials.data_ptr<double>(), wp(std::get<0>(out)), std::get<1>(out).data_ptr<int>(), (int)p.size(0), (int)p.size(1),
                                   (int)p.size(2), (int)g.size(1), (int)g.size(2), stream_of(pred.device())),
     "sgr_eval_depth_log_rmse");
  return out;
}
T2 eval_depth_log_rmse_meta(const Tensor& pred, const Tensor& gt) { return depth_alloc(std::get<0>(depth_views(pred, gt, false))); }

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("eval_whdr(Tensor reflectance, Tensor point, Tensor weight, Tensor label, Tensor num, float delta=0.1) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("eval_normal_angle(Tensor normalPred, Tensor normalGt, Tensor mask) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("eval_depth_log_rmse(Tensor depthPred, Tensor depthGt) -> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("eval_whdr", &eval_whdr_cuda);
  m.impl("eval_normal_angle", &eval_normal_angle_cuda);
  m.impl("eval_depth_log_rmse", &eval_depth_log_rmse_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("eval_whdr", &eval_whdr_meta);
  m.impl("eval_normal_angle", &eval_normal_angle_meta);
  m.impl("eval_depth_log_rmse", &eval_depth_log_rmse_meta);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"eval_whdr", "eval_normal_angle", "eval_depth_log_rmse"}); }

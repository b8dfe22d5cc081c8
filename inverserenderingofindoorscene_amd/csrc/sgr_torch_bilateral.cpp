// torch.ops.sgrender.bilateral_*: the bilateral solver layer (BilateralLayer.py:20-124) as operators of the C++ torch extension.
//
// Same rules as sgr_torch.cpp: every operator checks its arguments, allocates outputs and workspace with the caching allocator and
// calls the C ABI (sgr_bs_* of include/sgrender.h) on the current HIP stream; nothing here computes.  The one piece of plumbing is
// the sort of the pixel keys (at::sort, stable) between sgr_bs_grid_keys and sgr_bs_grid_build.  All shapes are static
// (nvertices <= H*W, the per-image count stays on the device), so the Meta functions need no data and nothing synchronises.
//
//   bilateral_grid        BilateralGrid.__init__ + bistochastize              BilateralGrid.py:43-118
//   bilateral_solve_fwd   BilateralGrid.solve                                 BilateralGrid.py:126-153,193-198
//   bilateral_solve_bwd   BilateralGrid.solveForGrad                          BilateralGrid.py:155-191,200-212
//   bilateral_solve       BilateralFunction (forward + autograd node; the grid built in forward is reused in backward)
#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;

void require_dev(std::initializer_list<const Tensor*> ts, const c10::Device& dev) {
  for (const Tensor* t : ts) {
    TORCH_CHECK(t->is_cuda(), kNoCpu);
    TORCH_CHECK(t->device() == dev, "sgrender: tensors on different devices (", dev, " vs ", t->device(), ")");
  }
}

struct Dims { int64_t B, C, H, W; };
void check_image(const Tensor& image) {
  TORCH_CHECK(image.dim() == 4 && image.size(1) == 3, "sgrender: the bilateral guide image must be [B,3,H,W], got ", image.sizes());
  TORCH_CHECK(image.scalar_type() == at::kFloat, "sgrender: fp32 tensors required, got ", image.scalar_type());
  TORCH_CHECK(image.numel() > 0, "sgrender: zero-sized bilateral guide image ", image.sizes());
}
Dims check_target(const Tensor& pred, const Tensor& conf, const Tensor& pix2vert) {
  TORCH_CHECK(pred.dim() == 4 && pred.size(1) >= 1 && pred.size(1) <= 3, "sgrender: the bilateral target must be [B,C,H,W] with C in 1..3, got ", pred.sizes());
  const int64_t B = pred.size(0), C = pred.size(1), H = pred.size(2), W = pred.size(3);
  TORCH_CHECK(conf.sizes() == at::IntArrayRef({B, 1, H, W}), "sgrender: the bilateral confidence must be [", B, ",1,", H, ",", W, "], got ", conf.sizes());
  TORCH_CHECK(pix2vert.sizes() == at::IntArrayRef({B, H * W}), "sgrender: the bilateral grid was built for another shape: ", pix2vert.sizes());
  TORCH_CHECK(pred.scalar_type() == at::kFloat && conf.scalar_type() == at::kFloat, "sgrender: fp32 tensors required");
  TORCH_CHECK(B > 0 && H > 0 && W > 0, "sgrender: zero-sized bilateral target ", pred.sizes());
  return {B, C, H, W};
}
void check_grid(const Tensor& pix2vert, const Tensor& perm, const Tensor& seg, const Tensor& nbr, const Tensor& nvert, const Tensor& m, const Tensor& n) {
  TORCH_CHECK(pix2vert.dim() == 2, "sgrender: pix2vert must be [B,H*W]");
  const int64_t B = pix2vert.size(0), N = pix2vert.size(1);
  TORCH_CHECK(perm.sizes() == pix2vert.sizes() && seg.sizes() == pix2vert.sizes() && nbr.sizes() == at::IntArrayRef({B, N, 10}) && nvert.sizes() == at::IntArrayRef({B}) &&
                  m.sizes() == pix2vert.sizes() && n.sizes() == pix2vert.sizes(),
              "sgrender: bilateral grid tensors of inconsistent shapes");
  for (const Tensor* t : {&pix2vert, &perm, &seg, &nbr, &nvert}) TORCH_CHECK(t->scalar_type() == at::kInt && t->is_contiguous(), "sgrender: bilateral grid index tensors must be contiguous int32");
  for (const Tensor* t : {&m, &n}) TORCH_CHECK(t->scalar_type() == at::kDouble && t->is_contiguous(), "sgrender: bilateral grid m / n must be contiguous fp64");
}

Tensor workspace(int64_t B, int64_t H, int64_t W, int64_t C, const at::TensorOptions& o) {
  const long long bytes = api().sgr_bs_workspace_bytes((int)B, (int)H, (int)W, (int)C);
  if (bytes < 0) ok((int)bytes, "sgr_bs_workspace_bytes");
  return at::empty({(int64_t)bytes}, o.dtype(at::kByte));
}

// ---- grid -------------------------------------------------------------------------------------------------------------
T7 grid_outputs(const Tensor& image) {
  const int64_t B = image.size(0), N = image.size(2) * image.size(3);
  const auto oi = image.options().dtype(at::kInt), od = image.options().dtype(at::kDouble);
  return {at::empty({B, N}, oi), at::empty({B, N}, oi), at::empty({B, N}, oi), at::empty({B, N, 10}, oi), at::empty({B}, oi), at::empty({B, N}, od), at::empty({B, N}, od)};
}
T7 bilateral_grid_cuda(const Tensor& image, double sl, double sc, double ss) {
  TORCH_CHECK(image.is_cuda(), kNoCpu);
  check_image(image);
  const auto dev = image.device();
  const c10::DeviceGuard guard(dev);
  const Tensor im = image.contiguous();
  const int64_t B = im.size(0), H = im.size(2), W = im.size(3);
  Tensor keys = at::empty({B * H * W}, im.options().dtype(at::kLong));
  ok(api().sgr_bs_grid_keys(im.const_data_ptr<float>(), (long long*)keys.data_ptr<int64_t>(), (int)B, (int)H, (int)W, sl, sc, ss, stream_of(dev)), "sgr_bs_grid_keys");
  auto [skeys, sidx] = at::sort(keys, /*stable=*/true, /*dim=*/0, /*descending=*/false);
  auto out = grid_outputs(im);
  Tensor ws = workspace(B, H, W, 1, im.options());
  ok(api().sgr_bs_grid_build((const long long*)skeys.const_data_ptr<int64_t>(), (const long long*)sidx.const_data_ptr<int64_t>(), std::get<0>(out).data_ptr<int>(),
                             std::get<1>(out).data_ptr<int>(), std::get<2>(out).data_ptr<int>(), std::get<3>(out).data_ptr<int>(), std::get<4>(out).data_ptr<int>(),
                             std::get<5>(out).data_ptr<double>(), std::get<6>(out).data_ptr<double>(), ws.data_ptr(), (int)B, (int)H, (int)W, stream_of(dev)),
     "sgr_bs_grid_build");
  return out;
}
T7 bilateral_grid_meta(const Tensor& image, double, double, double) {
  check_image(image);
  return grid_outputs(image);
}

// ---- solve ------------------------------------------------------------------------------------------------------------
#define GRID_ARGS const Tensor &pix2vert, const Tensor &perm, const Tensor &seg, const Tensor &nbr, const Tensor &nvert, const Tensor &m, const Tensor &n
#define GRID_PTRS pix2vert.const_data_ptr<int>(), perm.const_data_ptr<int>(), seg.const_data_ptr<int>(), nbr.const_data_ptr<int>(), nvert.const_data_ptr<int>(), \
                  m.const_data_ptr<double>(), n.const_data_ptr<double>()

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Dims check_solve_fwd(GRID_ARGS, const Tensor& pred, const Tensor& conf, bool device) {
  if (device) {
    TORCH_CHECK(pred.is_cuda(), kNoCpu);
    require_dev({&pix2vert, &perm, &seg, &nbr, &nvert, &m, &n, &conf}, pred.device());
  }
  check_grid(pix2vert, perm, seg, nbr, nvert, m, n);
  return check_target(pred, conf, pix2vert);
}
T2 solve_fwd_outputs(const Dims& d, const at::TensorOptions& o) { return {at::empty({d.B, d.C, d.H, d.W}, o), at::empty({d.B, d.H * d.W, d.C}, o.dtype(at::kDouble))}; }
T2 bilateral_solve_fwd_cuda(GRID_ARGS, const Tensor& pred, const Tensor& conf, double lam, double amin, double tol, int64_t maxiter) {
  const auto d = check_solve_fwd(pix2vert, perm, seg, nbr, nvert, m, n, pred, conf, true);
  const c10::DeviceGuard guard(pred.device());
  auto [out, yhat] = solve_fwd_outputs(d, pred.options());
  const Tensor t = pred.contiguous(), w = conf.contiguous();
  Tensor ws = workspace(d.B, d.H, d.W, d.C, t.options());
  ok(api().sgr_bs_solve_fwd(GRID_PTRS, t.const_data_ptr<float>(), w.const_data_ptr<float>(), out.data_ptr<float>(), yhat.data_ptr<double>(), ws.data_ptr(), (int)d.B,
                            (int)d.C, (int)d.H, (int)d.W, lam, amin, tol, (int)maxiter, stream_of(pred.device())),
     "sgr_bs_solve_fwd");
  return {out, yhat};
}
T2 bilateral_solve_fwd_meta(GRID_ARGS, const Tensor& pred, const Tensor& conf, double, double, double, int64_t) {
  return solve_fwd_outputs(check_solve_fwd(pix2vert, perm, seg, nbr, nvert, m, n, pred, conf, false), pred.options());
}

Dims check_solve_bwd(GRID_ARGS, const Tensor& g_out, const Tensor& pred, const Tensor& conf, const Tensor& yhat, bool device) {
  if (device) {
    TORCH_CHECK(pred.is_cuda(), kNoCpu);
    require_dev({&pix2vert, &perm, &seg, &nbr, &nvert, &m, &n, &conf, &g_out, &yhat}, pred.device());
  }
  check_grid(pix2vert, perm, seg, nbr, nvert, m, n);
  const auto d = check_target(pred, conf, pix2vert);
  TORCH_CHECK(g_out.sizes() == pred.sizes() && g_out.scalar_type() == at::kFloat, "sgrender: the bilateral cotangent must match the target: ", g_out.sizes());
  TORCH_CHECK(yhat.sizes() == at::IntArrayRef({d.B, d.H * d.W, d.C}) && yhat.scalar_type() == at::kDouble, "sgrender: yhat must be the fp64 [B,H*W,C] tensor of the forward solve");
  return d;
}
T2 solve_bwd_outputs(const Dims& d, const at::TensorOptions& o) { return {at::empty({d.B, d.C, d.H, d.W}, o), at::empty({d.B, 1, d.H, d.W}, o)}; }      // g_pred, g_conf
T2 bilateral_solve_bwd_cuda(GRID_ARGS, const Tensor& g_out, const Tensor& pred, const Tensor& conf, const Tensor& yhat, double lam, double amin, double tol,
                            int64_t maxiter) {
  const auto d = check_solve_bwd(pix2vert, perm, seg, nbr, nvert, m, n, g_out, pred, conf, yhat, true);
  const c10::DeviceGuard guard(pred.device());
  auto [gp, gc] = solve_bwd_outputs(d, pred.options());
  const Tensor g = g_out.contiguous(), t = pred.contiguous(), w = conf.contiguous(), yh = yhat.contiguous();
  Tensor ws = workspace(d.B, d.H, d.W, d.C, t.options());
  ok(api().sgr_bs_solve_bwd(GRID_PTRS, g.const_data_ptr<float>(), t.const_data_ptr<float>(), w.const_data_ptr<float>(), yh.const_data_ptr<double>(), gp.data_ptr<float>(),
                            gc.data_ptr<float>(), ws.data_ptr(), (int)d.B, (int)d.C, (int)d.H, (int)d.W, lam, amin, tol, (int)maxiter, stream_of(pred.device())),
     "sgr_bs_solve_bwd");
  return {gp, gc};
}
T2 bilateral_solve_bwd_meta(GRID_ARGS, const Tensor& g_out, const Tensor& pred, const Tensor& conf, const Tensor& yhat, double, double, double, int64_t) {
  return solve_bwd_outputs(check_solve_bwd(pix2vert, perm, seg, nbr, nvert, m, n, g_out, pred, conf, yhat, false), pred.options());
}

using GridSig = T7(const Tensor&, double, double, double);
using FwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, double, double, double,
                  int64_t);
using BwdSig = T2(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&,
                  const Tensor&, double, double, double, int64_t);

// the composite: grid + forward solve (device and Meta alike: both are made of registered operators)
Tensor bilateral_solve_impl(const Tensor& image, const Tensor& pred, const Tensor& conf, double sl, double sc, double ss, double lam, double amin, double tol, int64_t maxiter) {
  static auto grid = find_op<GridSig>("sgrender::bilateral_grid");
  static auto fwd = find_op<FwdSig>("sgrender::bilateral_solve_fwd");
  auto [p2v, perm, seg, nbr, nvert, m, n] = grid.call(image, sl, sc, ss);
  return std::get<0>(fwd.call(p2v, perm, seg, nbr, nvert, m, n, pred, conf, lam, amin, tol, maxiter));
}

struct BilateralSolveFn : public torch::autograd::Function<BilateralSolveFn> {
  static Tensor forward(AutogradContext* ctx, const Tensor& image, const Tensor& pred, const Tensor& conf, double sl, double sc, double ss, double lam, double amin,
                        double tol, int64_t maxiter) {
    at::AutoDispatchBelowADInplaceOrView guard;
    static auto grid = find_op<GridSig>("sgrender::bilateral_grid");
    static auto fwd = find_op<FwdSig>("sgrender::bilateral_solve_fwd");
    auto [p2v, perm, seg, nbr, nvert, m, n] = grid.call(image, sl, sc, ss);
    auto [out, yhat] = fwd.call(p2v, perm, seg, nbr, nvert, m, n, pred, conf, lam, amin, tol, maxiter);
    ctx->save_for_backward({p2v, perm, seg, nbr, nvert, m, n, pred, conf, yhat});
    ctx->saved_data["lam"] = lam;
    ctx->saved_data["amin"] = amin;
    ctx->saved_data["tol"] = tol;
    ctx->saved_data["maxiter"] = maxiter;
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    variable_list out(10);
    if (!g[0].defined()) return out;
    const auto s = ctx->get_saved_variables();
    static auto bwd = find_op<BwdSig>("sgrender::bilateral_solve_bwd");
    auto [gp, gc] = bwd.call(s[0], s[1], s[2], s[3], s[4], s[5], s[6], g[0], s[7], s[8], s[9], ctx->saved_data["lam"].toDouble(), ctx->saved_data["amin"].toDouble(),
                             ctx->saved_data["tol"].toDouble(), ctx->saved_data["maxiter"].toInt());
    out[1] = gp;     // no gradient to the guide image or the parameters (BilateralLayer.py:124)
    out[2] = gc;
    return out;
  }
};
Tensor bilateral_solve_autograd(const Tensor& image, const Tensor& pred, const Tensor& conf, double sl, double sc, double ss, double lam, double amin, double tol,
                                int64_t maxiter) {
  return BilateralSolveFn::apply(image, pred, conf, sl, sc, ss, lam, amin, tol, maxiter);
}

}  // namespace

#define GRID_SCHEMA "Tensor pix2vert, Tensor perm, Tensor seg, Tensor nbr, Tensor nvert, Tensor m, Tensor n"
TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("bilateral_grid(Tensor image, float sigma_luma, float sigma_chroma, float sigma_spatial) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("bilateral_solve_fwd(" GRID_SCHEMA ", Tensor pred, Tensor conf, float lam, float A_diag_min, float cg_tol, int cg_maxiter) -> (Tensor, Tensor)");
  m.def("bilateral_solve_bwd(" GRID_SCHEMA ", Tensor g_out, Tensor pred, Tensor conf, Tensor yhat, float lam, float A_diag_min, float cg_tol, int cg_maxiter) -> (Tensor, Tensor)");
  m.def("bilateral_solve(Tensor image, Tensor pred, Tensor conf, float sigma_luma, float sigma_chroma, float sigma_spatial, float lam, float A_diag_min, float cg_tol, "
        "int cg_maxiter) -> Tensor");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("bilateral_grid", &bilateral_grid_cuda);
  m.impl("bilateral_solve_fwd", &bilateral_solve_fwd_cuda);
  m.impl("bilateral_solve_bwd", &bilateral_solve_bwd_cuda);
  m.impl("bilateral_solve", &bilateral_solve_impl);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("bilateral_grid", &bilateral_grid_meta);
  m.impl("bilateral_solve_fwd", &bilateral_solve_fwd_meta);
  m.impl("bilateral_solve_bwd", &bilateral_solve_bwd_meta);
  m.impl("bilateral_solve", &bilateral_solve_impl);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) { m.impl("bilateral_solve", &bilateral_solve_autograd); }
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"bilateral_grid", "bilateral_solve_fwd", "bilateral_solve_bwd", "bilateral_solve"}); }

// torch.ops.sgrender.gn_stage_siblings / gn_resize_siblings and their _bwd operators: the decoder stage of sgr_torch_gn_stage.cpp and
// sgr_torch_gn_resize.cpp for D sibling decoders in one call.  The reference runs four decoder0 and three
// decoderLight instances on the same encoder features (wrapperBRDF.py:104-107, wrapperBRDFLight.py:104-115), so at a stage the siblings
// differ in x and in the dgnK parameters alone: same shapes, one skip.
//
// Same rules as the single operators' files: every operator checks its arguments, allocates its outputs and its workspace with the caching
// allocator and calls the C ABI (sgr_gn_stage_siblings_* / sgr_gn_resize_siblings_* of include/sgrender.h) on the current HIP stream; nothing
// here computes and nothing synchronises.  The siblings' pointers travel as host arrays into the kernel arguments: no device-side table.
// Where a list entry is "absent" (a sibling without a cotangent, an x the backward does not need, a gradient nobody wants) it is a [0] tensor.
#include <array>

#include "sgr_torch_common.hpp"

namespace {

using namespace sgr_host;
using OT = OptTensor;
using TL = at::TensorList;
using TV = std::vector<Tensor>;
using FwdOut = std::tuple<TV, Tensor>;
using BwdOut = std::tuple<TV, TV, TV, Tensor>;

constexpr int64_t kMaxSiblings = SGR_GN_MAX_SIBLINGS;

bool io_type(at::ScalarType t) { return t == at::kFloat || t == at::kBFloat16; }

struct Sib {
  int64_t D = 0, B = 0, C = 0, Cs = 0, H = 0, W = 0, Hs = 0, Ws = 0, G = 0;
  bool resize = false;
  const char* who = "";
  std::vector<int64_t> out_sizes() const { return {B, C + Cs, 2 * Hs, 2 * Ws}; }
};

constexpr const char* kOutside =
    "the fused resize covers H <= h <= 2H and W <= w <= 2W per axis (what floor-halving encoders and doubling decoders produce); any other "
    "size stays the caller's composition";

void check_sizes(const Sib& s) {
  TORCH_CHECK(s.D >= 1 && s.D <= kMaxSiblings, "sgrender: ", s.who, ": the number of siblings must be 1 .. ", kMaxSiblings, ", got ", s.D);
  TORCH_CHECK(s.B > 0 && s.C > 0 && s.H > 0 && s.W > 0, "sgrender: ", s.who, ": zero-sized x [", s.B, ",", s.C, ",", s.H, ",", s.W, "]");
  TORCH_CHECK(s.G > 0 && s.C % s.G == 0, "sgrender: ", s.who, ": the channel count ", s.C, " is not a multiple of num_groups ", s.G);
  TORCH_CHECK(s.Cs >= 1, "sgrender: ", s.who, ": the sibling forms need a skip with at least one channel");
  if (s.resize) {
    TORCH_CHECK(s.Hs >= s.H && s.Hs <= 2 * s.H && s.Ws >= s.W && s.Ws <= 2 * s.W, "sgrender: ", s.who, ": the skip ", s.Hs, "x", s.Ws, " is outside the resize domain of x ", s.H,
                "x", s.W, "; ", kOutside);
  } else {
    TORCH_CHECK(s.Hs == s.H && s.Ws == s.W, "sgrender: ", s.who, ": skip is ", s.Hs, "x", s.Ws, " but x is ", s.H, "x", s.W,
                "; gn_resize_siblings (group_norm_relu_resize_upcat_siblings) is the form that resizes the normalised maps to the skip");
  }
  TORCH_CHECK(s.B <= 65535 && s.D * s.C + s.Cs <= 65535 && s.D * s.G <= 65535 && s.Hs * s.Ws < (int64_t(1) << 26), "sgrender: ", s.who, ": size out of range");
}

// shared by the device and the Meta kernels: a traced graph cannot pass tracing and then fail on the device
Sib check_fwd(TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps, bool resize, bool device) {
  Sib s;
  s.resize = resize;
  s.who = resize ? "gn_resize_siblings" : "gn_stage_siblings";
  s.D = (int64_t)xs.size();
  TORCH_CHECK(s.D >= 1 && s.D <= kMaxSiblings, "sgrender: ", s.who, ": the number of siblings must be 1 .. ", kMaxSiblings, ", got ", s.D);
  TORCH_CHECK((int64_t)weights.size() == s.D && (int64_t)biases.size() == s.D, "sgrender: ", s.who, ": ", s.D, " xs but ", weights.size(), " weights and ", biases.size(),
              " biases");
  TORCH_CHECK(skip.defined(), "sgrender: ", s.who, ": the sibling forms need a skip");
  const Tensor& x0 = xs[0];
  TORCH_CHECK(x0.dim() == 4, "sgrender: ", s.who, ": xs[0] must be [B,C,H,W], got ", x0.sizes());
  for (int64_t d = 0; d < s.D; ++d) {
    if (device) TORCH_CHECK(xs[d].is_cuda() && weights[d].is_cuda() && biases[d].is_cuda() && skip.is_cuda(), kNoCpu);
    TORCH_CHECK(xs[d].sizes() == x0.sizes(), "sgrender: ", s.who, ": the siblings must have one shape, got xs[0] ", x0.sizes(), " and xs[", d, "] ", xs[d].sizes());
    TORCH_CHECK(xs[d].scalar_type() == x0.scalar_type(), "sgrender: ", s.who, ": the siblings must have one dtype, got xs[0] ", x0.scalar_type(), " and xs[", d, "] ",
                xs[d].scalar_type());
    TORCH_CHECK(xs[d].device() == x0.device() && weights[d].device() == x0.device() && biases[d].device() == x0.device() && skip.device() == x0.device(), "sgrender: ",
                s.who, ": tensors on different devices");
  }
  const auto xt = x0.scalar_type();
  if (resize) {
    TORCH_CHECK(xt == at::kFloat && skip.scalar_type() == at::kFloat, "sgrender: ", s.who, ": fp32 tensors required (xs ", xt, ", skip ", skip.scalar_type(), ")");
  } else {
    TORCH_CHECK(io_type(xt), "sgrender: ", s.who, ": fp32 tensors required (xs ", xt, ", skip ", skip.scalar_type(), ")");
    TORCH_CHECK(skip.scalar_type() == xt, "sgrender: ", s.who, ": xs and skip must have one dtype, got xs ", xt, " and skip ", skip.scalar_type(),
                "; cast one of them (under torch.autocast the operator casts skip to the dtype of xs itself)");
  }
  s.B = x0.size(0); s.C = x0.size(1); s.H = x0.size(2); s.W = x0.size(3); s.G = G;
  TORCH_CHECK(skip.dim() == 4 && skip.size(0) == s.B && skip.size(1) >= 1, "sgrender: ", s.who, ": skip must be [", s.B, ",Cs,h,w] with Cs >= 1, got ", skip.sizes());
  s.Cs = skip.size(1); s.Hs = skip.size(2); s.Ws = skip.size(3);
  check_sizes(s);
  for (int64_t d = 0; d < s.D; ++d)
    TORCH_CHECK(weights[d].scalar_type() == at::kFloat && biases[d].scalar_type() == at::kFloat && weights[d].dim() == 1 && biases[d].dim() == 1 &&
                    weights[d].size(0) == s.C && biases[d].size(0) == s.C,
                "sgrender: ", s.who, ": weights and biases must be fp32 [", s.C, "] (the parameters stay fp32, as under torch.autocast), got ", weights[d].scalar_type(), " ",
                weights[d].sizes(), " and ", biases[d].scalar_type(), " ", biases[d].sizes(), " for sibling ", d);
  TORCH_CHECK(eps > 0, "sgrender: ", s.who, ": eps must be positive");
  return s;
}

// D device pointers and D x 4 strides for the C ABI, which reads them during the call
struct Ptrs {
  std::array<const void*, SGR_GN_MAX_SIBLINGS> p{};
  template <typename T> const T* const* in() const { return reinterpret_cast<const T* const*>(p.data()); }
  template <typename T> T* const* out() const { return (T* const*)p.data(); }      // the outputs were taken with const_data_ptr to share ptrs_of
};
Ptrs ptrs_of(const TV& ts) {
  Ptrs r;
  for (size_t d = 0; d < ts.size(); ++d) r.p[d] = present(ts[d]) ? ts[d].const_data_ptr() : nullptr;
  return r;
}
std::vector<long long> strides_of(TL xs) {
  std::vector<long long> v(4 * xs.size(), 0);
  for (size_t d = 0; d < xs.size(); ++d)
    if (present(xs[d]))
      for (int k = 0; k < 4; ++k) v[4 * d + k] = (long long)xs[d].stride(k);
  return v;
}
TV contiguous(TL ts) {
  TV r;
  for (const Tensor& t : ts) r.push_back(present(t) ? t.contiguous() : t);
  return r;
}

Tensor workspace(const Sib& s, bool backward, const at::TensorOptions& of) {
  return workspace_floats(s.resize ? api().sgr_gn_resize_siblings_workspace_floats((int)s.D, (int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, (int)s.Hs, (int)s.Ws, backward)
                               : api().sgr_gn_stage_siblings_workspace_floats((int)s.D, (int)s.B, (int)s.C, (int)s.G, (int)s.H, (int)s.W, backward), s.who, of);
}

// -> (outs, stats [D,B,G,4])
FwdOut fwd_cuda(TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps, bool resize) {
  const Sib s = check_fwd(xs, weights, biases, skip, G, eps, resize, true);
  const c10::DeviceGuard guard(skip.device());
  const auto o = xs[0].options().memory_format(at::MemoryFormat::Contiguous), of = o.dtype(at::kFloat);
  TV outs;
  for (int64_t d = 0; d < s.D; ++d) outs.push_back(at::empty(s.out_sizes(), o));
  Tensor stats = at::empty({s.D, s.B, s.G, 4}, of);
  const TV w = contiguous(weights), b = contiguous(biases);
  const Tensor ws = workspace(s, false, of);
  const Ptrs px = ptrs_of(xs.vec()), pw = ptrs_of(w), pb = ptrs_of(b), po = ptrs_of(outs);
  const std::vector<long long> xst = strides_of(xs);
  const long long sst[4] = {(long long)skip.stride(0), (long long)skip.stride(1), (long long)skip.stride(2), (long long)skip.stride(3)};
  void* st = stream_of(skip.device());
  if (resize) {
    ok(api().sgr_gn_resize_siblings_fwd((int)s.D, px.in<float>(), pw.in<float>(), pb.in<float>(), rp(skip), po.out<float>(), wp(stats), wp(ws), (int)s.B, (int)s.C,
                                        (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, (int)s.Hs, (int)s.Ws, xst.data(), sst, (float)eps, st),
       "sgr_gn_resize_siblings_fwd");
  } else if (xs[0].scalar_type() == at::kBFloat16) {
    ok(api().sgr_gn_stage_siblings_fwd_bf16((int)s.D, px.in<unsigned short>(), pw.in<float>(), pb.in<float>(), static_cast<const unsigned short*>(skip.const_data_ptr()),
                                            po.out<unsigned short>(), wp(stats), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, xst.data(), sst,
                                            (float)eps, st),
       "sgr_gn_stage_siblings_fwd_bf16");
  } else {
    ok(api().sgr_gn_stage_siblings_fwd((int)s.D, px.in<float>(), pw.in<float>(), pb.in<float>(), rp(skip), po.out<float>(), wp(stats), wp(ws), (int)s.B, (int)s.C,
                                       (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, xst.data(), sst, (float)eps, st),
       "sgr_gn_stage_siblings_fwd");
  }
  return {outs, stats};
}
FwdOut fwd_meta(TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps, bool resize) {
  const Sib s = check_fwd(xs, weights, biases, skip, G, eps, resize, false);
  const auto o = xs[0].options().memory_format(at::MemoryFormat::Contiguous);
  TV outs;
  for (int64_t d = 0; d < s.D; ++d) outs.push_back(at::empty(s.out_sizes(), o));
  return {outs, at::empty({s.D, s.B, s.G, 4}, o.dtype(at::kFloat))};
}
FwdOut gn_stage_siblings_cuda(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return fwd_cuda(xs, w, b, skip, G, eps, false); }
FwdOut gn_stage_siblings_meta(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return fwd_meta(xs, w, b, skip, G, eps, false); }
FwdOut gn_resize_siblings_cuda(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return fwd_cuda(xs, w, b, skip, G, eps, true); }
FwdOut gn_resize_siblings_meta(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return fwd_meta(xs, w, b, skip, G, eps, true); }

// The backward's checks.  nX / nW / nB: bit d set = sibling d's gradient is wanted; a sibling whose cotangent is absent gets none (the
// bits are cleared here).  xs / weights / biases of a sibling that gets none may be [0]; H, W: the sizes of the xs.
Sib check_bwd(TL gs, TL xs, TL weights, TL biases, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, int64_t& nX, int64_t& nW, int64_t& nB, bool nS,
              bool resize, bool device) {
  Sib s;
  s.resize = resize;
  s.who = resize ? "gn_resize_siblings_bwd" : "gn_stage_siblings_bwd";
  s.D = (int64_t)gs.size();
  TORCH_CHECK(s.D >= 1 && s.D <= kMaxSiblings, "sgrender: ", s.who, ": the number of siblings must be 1 .. ", kMaxSiblings, ", got ", s.D);
  TORCH_CHECK((int64_t)xs.size() == s.D && (int64_t)weights.size() == s.D && (int64_t)biases.size() == s.D, "sgrender: ", s.who, ": ", s.D, " cotangents but ", xs.size(),
              " xs, ", weights.size(), " weights and ", biases.size(), " biases");
  const Tensor* g0 = nullptr;
  for (int64_t d = 0; d < s.D; ++d) {
    if (!present(gs[d])) {
      nX &= ~(int64_t(1) << d); nW &= ~(int64_t(1) << d); nB &= ~(int64_t(1) << d);
      continue;
    }
    if (!g0) g0 = &gs[d];
    if (device) TORCH_CHECK(gs[d].is_cuda(), kNoCpu);
    TORCH_CHECK(gs[d].sizes() == g0->sizes() && gs[d].scalar_type() == g0->scalar_type() && gs[d].device() == g0->device(), "sgrender: ", s.who,
                ": the cotangents must have one shape, dtype and device");
  }
  TORCH_CHECK(g0, "sgrender: ", s.who, ": no cotangent given");
  const int64_t all = (int64_t(1) << s.D) - 1;
  TORCH_CHECK((nX & ~all) == 0 && (nW & ~all) == 0 && (nB & ~all) == 0, "sgrender: ", s.who, ": a gradient requested for a sibling that does not exist");
  TORCH_CHECK(nX || nW || nB || nS, "sgrender: ", s.who, ": no gradient requested");
  const auto gt = g0->scalar_type();
  TORCH_CHECK(g0->dim() == 4 && (resize ? gt == at::kFloat : io_type(gt)) && C > 0 && Cs > 0 && g0->size(1) == C + Cs, "sgrender: ", s.who, ": the cotangents must be ",
              resize ? "fp32" : "fp32 or bf16", " [B,", C + Cs, ",.,.], got ", gt, " ", g0->sizes());
  s.B = g0->size(0); s.C = C; s.Cs = Cs; s.G = G; s.H = H; s.W = W;
  s.Hs = g0->size(2) / 2; s.Ws = g0->size(3) / 2;
  TORCH_CHECK(g0->sizes() == at::IntArrayRef(s.out_sizes()), "sgrender: ", s.who, ": the cotangent of an upsampled result must have even sizes, got ", g0->sizes());
  check_sizes(s);
  if (nX || nW || nB) {
    TORCH_CHECK(stats.has_value() && stats->defined(), "sgrender: ", s.who, ": xs, weights, biases and stats are needed for dx, dweight and dbias");
    if (device) TORCH_CHECK(stats->is_cuda(), kNoCpu);
    TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->sizes() == at::IntArrayRef({s.D, s.B, s.G, 4}), "sgrender: ", s.who, ": stats must be fp32 [", s.D, ",", s.B, ",",
                s.G, ",4], got ", stats->sizes());
  }
  for (int64_t d = 0; d < s.D; ++d) {
    if (!(((nX | nW | nB) >> d) & 1)) continue;
    TORCH_CHECK(present(xs[d]) && present(weights[d]) && present(biases[d]), "sgrender: ", s.who, ": xs, weights, biases and stats are needed for dx, dweight and dbias");
    if (device) TORCH_CHECK(xs[d].is_cuda() && weights[d].is_cuda() && biases[d].is_cuda(), kNoCpu);
    TORCH_CHECK(xs[d].scalar_type() == gt && xs[d].sizes() == at::IntArrayRef({s.B, s.C, s.H, s.W}), "sgrender: ", s.who, ": xs[", d, "] must be ", gt, " [", s.B, ",", s.C, ",",
                s.H, ",", s.W, "], got ", xs[d].scalar_type(), " ", xs[d].sizes());
    TORCH_CHECK(weights[d].scalar_type() == at::kFloat && biases[d].scalar_type() == at::kFloat && weights[d].dim() == 1 && biases[d].dim() == 1 &&
                    weights[d].size(0) == s.C && biases[d].size(0) == s.C,
                "sgrender: ", s.who, ": weights and biases must be fp32 [", s.C, "]");
  }
  return s;
}
// a [0] tensor where a gradient is not wanted; dx and dskip in the cotangents' dtype (o), dweight and dbias in fp32
BwdOut bwd_outputs(const Sib& s, const at::TensorOptions& o, int64_t nX, int64_t nW, int64_t nB, bool nS) {
  const auto of = o.dtype(at::kFloat);
  TV dx, dw, db;
  for (int64_t d = 0; d < s.D; ++d) {
    dx.push_back(at::empty(((nX >> d) & 1) ? std::vector<int64_t>{s.B, s.C, s.H, s.W} : std::vector<int64_t>{0}, o));
    dw.push_back(at::empty({((nW >> d) & 1) ? s.C : 0}, of));
    db.push_back(at::empty({((nB >> d) & 1) ? s.C : 0}, of));
  }
  return {dx, dw, db, at::empty(nS ? std::vector<int64_t>{s.B, s.Cs, s.Hs, s.Ws} : std::vector<int64_t>{0}, o)};
}
const at::TensorOptions options_of(TL gs) {
  for (const Tensor& g : gs)
    if (present(g)) return g.options().memory_format(at::MemoryFormat::Contiguous);
  return at::TensorOptions();
}

BwdOut bwd_cuda(TL gs, TL xs, TL weights, TL biases, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, int64_t nX, int64_t nW, int64_t nB, bool nS,
                bool resize) {
  const Sib s = check_bwd(gs, xs, weights, biases, stats, C, Cs, G, H, W, nX, nW, nB, nS, resize, true);
  const auto o = options_of(gs);
  const c10::DeviceGuard guard(o.device());
  const bool side = nX || nW || nB;
  BwdOut out = bwd_outputs(s, o, nX, nW, nB, nS);
  const TV gc = contiguous(gs), w = contiguous(weights), b = contiguous(biases);
  Tensor st, ws;
  if (side) {
    st = stats->contiguous();
    ws = workspace(s, true, o.dtype(at::kFloat));
  }
  const Ptrs pg = ptrs_of(gc), px = ptrs_of(xs.vec()), pw = ptrs_of(w), pb = ptrs_of(b), pdx = ptrs_of(std::get<0>(out)), pdw = ptrs_of(std::get<1>(out)),
             pdb = ptrs_of(std::get<2>(out));
  const std::vector<long long> xst = strides_of(xs);
  const Tensor& ds = std::get<3>(out);
  void* stream = stream_of(o.device());
  if (resize) {
    ok(api().sgr_gn_resize_siblings_bwd((int)s.D, pg.in<float>(), px.in<float>(), pw.in<float>(), pb.in<float>(), rp(st), pdx.out<float>(), pdw.out<float>(),
                                        pdb.out<float>(), wp(ds), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, (int)s.Hs, (int)s.Ws, xst.data(),
                                        stream),
       "sgr_gn_resize_siblings_bwd");
  } else if (o.dtype() == at::kBFloat16) {
    ok(api().sgr_gn_stage_siblings_bwd_bf16((int)s.D, pg.in<unsigned short>(), px.in<unsigned short>(), pw.in<float>(), pb.in<float>(), rp(st), pdx.out<unsigned short>(),
                                            pdw.out<float>(), pdb.out<float>(), present(ds) ? static_cast<unsigned short*>(ds.mutable_data_ptr()) : nullptr, wp(ws),
                                            (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, xst.data(), stream),
       "sgr_gn_stage_siblings_bwd_bf16");
  } else {
    ok(api().sgr_gn_stage_siblings_bwd((int)s.D, pg.in<float>(), px.in<float>(), pw.in<float>(), pb.in<float>(), rp(st), pdx.out<float>(), pdw.out<float>(),
                                       pdb.out<float>(), wp(ds), wp(ws), (int)s.B, (int)s.C, (int)s.G, (int)s.Cs, (int)s.H, (int)s.W, xst.data(), stream),
       "sgr_gn_stage_siblings_bwd");
  }
  return out;
}
BwdOut bwd_meta(TL gs, TL xs, TL weights, TL biases, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, int64_t nX, int64_t nW, int64_t nB, bool nS,
                bool resize) {
  const Sib s = check_bwd(gs, xs, weights, biases, stats, C, Cs, G, H, W, nX, nW, nB, nS, resize, false);
  return bwd_outputs(s, options_of(gs), nX, nW, nB, nS);
}
#define SIB_BWD_ARGS TL gs, TL xs, TL w, TL b, const OT& stats, int64_t C, int64_t Cs, int64_t G, int64_t H, int64_t W, int64_t nX, int64_t nW, int64_t nB, bool nS
#define SIB_BWD_PASS gs, xs, w, b, stats, C, Cs, G, H, W, nX, nW, nB, nS
BwdOut gn_stage_siblings_bwd_cuda(SIB_BWD_ARGS) { return bwd_cuda(SIB_BWD_PASS, false); }
BwdOut gn_stage_siblings_bwd_meta(SIB_BWD_ARGS) { return bwd_meta(SIB_BWD_PASS, false); }
BwdOut gn_resize_siblings_bwd_cuda(SIB_BWD_ARGS) { return bwd_cuda(SIB_BWD_PASS, true); }
BwdOut gn_resize_siblings_bwd_meta(SIB_BWD_ARGS) { return bwd_meta(SIB_BWD_PASS, true); }

using FwdSig = FwdOut(TL, TL, TL, const Tensor&, int64_t, double);
using BwdSig = BwdOut(TL, TL, TL, TL, const OT&, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, bool);

const char* fwd_name(bool resize) { return resize ? "sgrender::gn_resize_siblings" : "sgrender::gn_stage_siblings"; }

// One node for all D siblings.  Inputs: D xs, D weights, D biases, skip; outputs: D results and the statistics.
struct GnSiblingsFn : public torch::autograd::Function<GnSiblingsFn> {
  static variable_list forward(AutogradContext* ctx, TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps, bool resize, int64_t nX, int64_t nW,
                               int64_t nB, bool nS) {
    FwdOut out;
    {
      at::AutoDispatchBelowADInplaceOrView guard;
      out = find_op<FwdSig>(fwd_name(resize)).call(xs, weights, biases, skip, G, eps);
    }
    // per sibling what gn_stage's node keeps -- x and the parameters where something behind the normalisation is wanted -- and the
    // statistics of all; y is recomputed, and skip is not kept: its gradient is linear in the cotangents
    const int64_t D = (int64_t)xs.size(), side = nX | nW | nB;
    variable_list keep;
    for (int64_t d = 0; d < D; ++d) {
      const bool k = (side >> d) & 1;
      keep.push_back(k ? xs[d] : Tensor());
      keep.push_back(k ? weights[d] : Tensor());
      keep.push_back(k ? biases[d] : Tensor());
    }
    keep.push_back(side ? std::get<1>(out) : Tensor());
    ctx->save_for_backward(keep);
    ctx->saved_data["D"] = D;
    ctx->saved_data["C"] = xs[0].size(1);
    ctx->saved_data["H"] = xs[0].size(2);
    ctx->saved_data["W"] = xs[0].size(3);
    ctx->saved_data["Cs"] = skip.size(1);
    ctx->saved_data["G"] = G;
    ctx->saved_data["resize"] = resize;
    ctx->saved_data["nX"] = nX; ctx->saved_data["nW"] = nW; ctx->saved_data["nB"] = nB; ctx->saved_data["nS"] = nS;
    ctx->mark_non_differentiable({std::get<1>(out)});
    ctx->set_materialize_grads(false);      // a result left out of the loss arrives undefined in backward, not as a map of zeros
    variable_list r = std::get<0>(out);
    r.push_back(std::get<1>(out));
    return r;
  }
  static variable_list backward(AutogradContext* ctx, variable_list g) {
    const int64_t D = ctx->saved_data["D"].toInt();
    variable_list out(3 * D + 8);
    const auto s = ctx->get_saved_variables();
    int64_t nX = ctx->saved_data["nX"].toInt(), nW = ctx->saved_data["nW"].toInt(), nB = ctx->saved_data["nB"].toInt();
    const bool nS = ctx->saved_data["nS"].toBool(), resize = ctx->saved_data["resize"].toBool();
    // a sibling left out of the loss has an undefined cotangent: no gradients for it, and it is left out of dskip's sum
    TV gs, xs, ws, bs;
    Tensor none;
    int64_t have = 0;
    for (int64_t d = 0; d < D; ++d)
      if (g[d].defined()) {
        have |= int64_t(1) << d;
        if (!none.defined()) none = at::empty({0}, g[d].options());
      }
    nX &= have; nW &= have; nB &= have;
    if (!have || !(nX || nW || nB || nS)) return out;
    for (int64_t d = 0; d < D; ++d) {
      const bool k = ((nX | nW | nB) >> d) & 1;
      gs.push_back(g[d].defined() ? g[d] : none);
      xs.push_back(k ? s[3 * d] : none);
      ws.push_back(k ? s[3 * d + 1] : none);
      bs.push_back(k ? s[3 * d + 2] : none);
    }
    const Tensor& st = s[3 * D];
    static auto bwd_stage = find_op<BwdSig>("sgrender::gn_stage_siblings_bwd");
    static auto bwd_resize = find_op<BwdSig>("sgrender::gn_resize_siblings_bwd");
    auto [dx, dw, db, ds] = (resize ? bwd_resize : bwd_stage)
                                .call(gs, xs, ws, bs, st.defined() ? OT(st) : OT(), ctx->saved_data["C"].toInt(), ctx->saved_data["Cs"].toInt(), ctx->saved_data["G"].toInt(),
                                      ctx->saved_data["H"].toInt(), ctx->saved_data["W"].toInt(), nX, nW, nB, nS);
    for (int64_t d = 0; d < D; ++d) {
      if ((nX >> d) & 1) out[d] = dx[d];
      if ((nW >> d) & 1) out[D + d] = dw[d];
      if ((nB >> d) & 1) out[2 * D + d] = db[d];
    }
    if (nS) out[3 * D] = ds;
    return out;
  }
};

FwdOut siblings_autograd(TL xs, TL weights, TL biases, const Tensor& skip, int64_t G, double eps, bool resize) {
  const bool grad = at::GradMode::is_enabled();
  int64_t nX = 0, nW = 0, nB = 0;
  const size_t D = std::min({xs.size(), weights.size(), biases.size(), (size_t)kMaxSiblings});      // the operator below refuses lists that do not agree
  for (size_t d = 0; grad && d < D; ++d) {
    nX |= int64_t(xs[d].requires_grad()) << d;
    nW |= int64_t(weights[d].requires_grad()) << d;
    nB |= int64_t(biases[d].requires_grad()) << d;
  }
  const bool nS = grad && skip.defined() && skip.requires_grad();
  const bool agree = xs.size() == weights.size() && xs.size() == biases.size() && xs.size() >= 1 && xs.size() <= (size_t)kMaxSiblings && skip.defined();
  if (!agree || !(nX || nW || nB || nS)) {      // nothing to differentiate (or a call the operator refuses): no node, nothing saved
    at::AutoDispatchBelowADInplaceOrView guard;
    return find_op<FwdSig>(fwd_name(resize)).call(xs, weights, biases, skip, G, eps);
  }
  auto o = GnSiblingsFn::apply(xs, weights, biases, skip, G, eps, resize, nX, nW, nB, nS);
  const Tensor stats = o.back();
  o.pop_back();
  return {o, stats};
}
FwdOut gn_stage_siblings_autograd(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return siblings_autograd(xs, w, b, skip, G, eps, false); }
FwdOut gn_resize_siblings_autograd(TL xs, TL w, TL b, const Tensor& skip, int64_t G, double eps) { return siblings_autograd(xs, w, b, skip, G, eps, true); }

}  // namespace

TORCH_LIBRARY_FRAGMENT(sgrender, m) {
  m.def("gn_stage_siblings(Tensor[] xs, Tensor[] weights, Tensor[] biases, Tensor skip, int num_groups, float eps=1e-05) -> (Tensor[], Tensor)");
  m.def("gn_resize_siblings(Tensor[] xs, Tensor[] weights, Tensor[] biases, Tensor skip, int num_groups, float eps=1e-05) -> (Tensor[], Tensor)");
  m.def("gn_stage_siblings_bwd(Tensor[] gs, Tensor[] xs, Tensor[] weights, Tensor[] biases, Tensor? stats, int channels, int skip_channels, int num_groups, int height, "
        "int width, int need_x, int need_weight, int need_bias, bool need_skip) -> (Tensor[], Tensor[], Tensor[], Tensor)");
  m.def("gn_resize_siblings_bwd(Tensor[] gs, Tensor[] xs, Tensor[] weights, Tensor[] biases, Tensor? stats, int channels, int skip_channels, int num_groups, int height, "
        "int width, int need_x, int need_weight, int need_bias, bool need_skip) -> (Tensor[], Tensor[], Tensor[], Tensor)");
}
TORCH_LIBRARY_IMPL(sgrender, CUDA, m) {
  m.impl("gn_stage_siblings", &gn_stage_siblings_cuda);
  m.impl("gn_resize_siblings", &gn_resize_siblings_cuda);
  m.impl("gn_stage_siblings_bwd", &gn_stage_siblings_bwd_cuda);
  m.impl("gn_resize_siblings_bwd", &gn_resize_siblings_bwd_cuda);
}
TORCH_LIBRARY_IMPL(sgrender, Meta, m) {
  m.impl("gn_stage_siblings", &gn_stage_siblings_meta);
  m.impl("gn_resize_siblings", &gn_resize_siblings_meta);
  m.impl("gn_stage_siblings_bwd", &gn_stage_siblings_bwd_meta);
  m.impl("gn_resize_siblings_bwd", &gn_resize_siblings_bwd_meta);
}
TORCH_LIBRARY_IMPL(sgrender, Autograd, m) {
  m.impl("gn_stage_siblings", &gn_stage_siblings_autograd);
  m.impl("gn_resize_siblings", &gn_resize_siblings_autograd);
}
TORCH_LIBRARY_IMPL(sgrender, CPU, m) { register_no_cpu(m, {"gn_stage_siblings", "gn_resize_siblings", "gn_stage_siblings_bwd", "gn_resize_siblings_bwd"}); }

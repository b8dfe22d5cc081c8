// Host-side plumbing shared by the C-ABI entry points: the error path, and the choice of a kernel's template arguments at run time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/sgrender.h"

namespace sgr {
void set_error(const char* msg);
int sgr_check(int hip_rc, const char* who);
void note_pending_error();

// The env-statistics fold of the fused light objective (recon_fold0_image, sgr_recon_fold.h) as a side job of the render loss's first pass:
// one extra workgroup per image.  ws == nullptr: no job.
struct FoldJob { const float* ws; float* coef; float* den_img; int nblk; };
// the three render-loss passes (sgr_loss.hip), shared by sgr_render_loss_fwd_total(_grads) and sgr_light_objective_fwd (sgr_fused_recon.hip)
int render_loss_fwd_launch(const float* diffuse, const float* spec, const float* im, const float* seg, float* im_small, float* seg_small,
                           float* rendered, float* coef, float* parts, float* loss, float* scale, float divisor, float weight,
                           float* g_diffuse, float* g_spec, float* workspace, int bn, int R, int C, int imH, int imW, FoldJob job, void* stream);
}  // namespace sgr

// Every entry point starts with SGR_REQUIRE.  Its first act is note_pending_error(): a (non-sticky) HIP error some earlier
// call on this thread left pending -- ours or another library's -- is taken off the error slot so that the hipGetLastError()
// after OUR launch reports our launch and nothing else, but it is not discarded: it is remembered (thread-local) and
// appended to the message of the next failure this library reports, and sgr_last_error() shows it until then.
#define SGR_REQUIRE(cond, msg)          \
  do {                                  \
    ::sgr::note_pending_error();        \
    if (!(cond)) {                      \
      ::sgr::set_error(msg);            \
      return SGR_ERR_BAD_ARG;           \
    }                                   \
  } while (0)

#define SGR_SUPPORTED(cond, msg)        \
  do {                                  \
    if (!(cond)) {                      \
      ::sgr::set_error(msg);            \
      return SGR_ERR_UNSUPPORTED;       \
    }                                   \
  } while (0)

namespace sgr {
// A run-time value chosen between two template arguments: f is a generic lambda whose parameter carries the constant,
//   with_flag(vec, [&](auto VEC) { hipLaunchKernelGGL((kernel<VEC()>), ...); });
// Both branches are instantiated, exactly as by the if / else this replaces.  Two run-time values nest the helper.  with_pool and
// with_ew (sgr_layer_launch.h) are the render layer's choices, built on `choose`.
template <int N> using Int = std::integral_constant<int, N>;
template <class A, class B, class F> static inline auto choose(bool first, F&& f) { return first ? f(A{}) : f(B{}); }
template <class F> static inline auto with_flag(bool on, F&& f) { return choose<std::true_type, std::false_type>(on, f); }
}  // namespace sgr

// SGR_GENERIC=1 forces the table-driven generic kernels (tuning / test knob); read once per process
static inline bool sgr_generic_forced() {
  static const bool on = [] { const char* e = getenv("SGR_GENERIC"); return e != nullptr && e[0] != 0 && !(e[0] == '0' && e[1] == 0); }();
  return on;
}

namespace sgr {
// Where the parts of the direction table start, in floats (include/sgrender.h): [Jpad][4] (lx, ly, lz, omega) with J = eh * ew padded
// to 32 | the separable rows [eh rounded up to even][8] | the separable columns, 8 * ew floats.  sgr_fill_direction_table (sgr_api.hip)
// writes by it and layer_dims (sgr_layer_launch.h) points the kernels into it; the offsets INSIDE the column block (cols + ew,
// cols + 4 * ew) belong to the kernels that read it (sgr_pk.inl) and to the writer's comments.
struct DirLayout { int Jpad, rows, cols, floats; };
static inline int dirs_padded(int J) { return (J + 31) / 32 * 32; }
static inline DirLayout dir_layout(int eh, int ew) {
  DirLayout t;
  t.Jpad = dirs_padded(eh * ew);
  t.rows = 4 * t.Jpad;
  t.cols = t.rows + 8 * ((eh + 1) / 2 * 2);
  t.floats = t.cols + 8 * ew;
  return t;
}

// BRDF maps, image and object mask come at the env grid's size or at twice it (POOL = 1 | 2: the kernels average 2x2 on the fly)
static inline bool pool1(int R, int C, int imH, int imW) { return imH == R && imW == C; }
static inline int check_pool(int R, int C, int imH, int imW, const char* who) {
  SGR_SUPPORTED(pool1(R, C, imH, imW) || (imH == 2 * R && imW == 2 * C), who);
  return SGR_OK;
}
}  // namespace sgr

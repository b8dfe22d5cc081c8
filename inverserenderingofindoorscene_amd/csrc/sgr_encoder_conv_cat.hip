// The several-source weight gradient of the encoders' convolution (sgr_encoder_conv_cat_bwd of sgr_encoder_conv.hip): the instantiations of
// ec_bwd_w_kernel that read the channels through a source table, in a translation unit of their own (sgr_encoder_conv_wgrad.inl says why).
#include "sgr_encoder_conv_wgrad.inl"

namespace sgr {

void ec_launch_w_cat(dim3 grid, hipStream_t st, int NT, int CW, const float* g, const EcSources& tab, float* partial, int C, int O, int H, int W, int tilesX,
                     int tiles, int opasses, int mode) {
#define EC_W(N, K) hipLaunchKernelGGL((ec_bwd_w_kernel<N, K, EcSources>), grid, dim3(kEcThreads), 0, st, g, (const float*)nullptr, EcStrides{}, partial, C, O, H, W, tilesX, tiles, opasses, mode, tab)
#define EC_W_N(N) do { if (CW == 1) EC_W(N, 1); else if (CW == 2) EC_W(N, 2); else if (CW == 3) EC_W(N, 3); else EC_W(N, 4); } while (0)
  if (NT == 1) EC_W_N(1); else if (NT == 2) EC_W_N(2); else if (NT == 3) EC_W_N(3); else EC_W_N(4);
#undef EC_W_N
#undef EC_W
}

}  // namespace sgr

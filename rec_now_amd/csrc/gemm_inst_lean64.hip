// Lean (interior-only) instantiations of the 256x64 tile family: (B,S)x(S,S)-like products and CIN's N = F product.
#include "gemm_kernel.hpp"

int rn_gemm_launch_lean64(const GemmK& k, bool a_kc, bool b_kc, int a2k, int b2k, dim3 grid, hipStream_t st) {
#define X(AKC, BKC, A2, B2)                                                                                          \
    if (a_kc == AKC && b_kc == BKC && a2k == A2 && b2k == B2) {                                                      \
        rn_gemm_launch_one<256, 64, 4, 1, 32, AKC, BKC, false, A2, B2>(k, grid, st);                                 \
        RN_LAUNCH_CHECK();                                                                                           \
        return RECNOW_OK;                                                                                            \
    }
    RN_GEMM_LEAN64_LIST(X)
#undef X
    return RN_EINTERNAL;
}

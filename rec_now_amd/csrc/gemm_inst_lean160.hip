// Lean (interior-only, compile-time operand kinds) instantiations of the 128x160 tile family.
#include "gemm_kernel.hpp"

int rn_gemm_launch_lean160(const GemmK& k, bool a_kc, bool b_kc, int bk, int a2k, int b2k, dim3 grid, hipStream_t st) {
#define X(AKC, BKC, A2, B2)                                                                                          \
    if (a_kc == AKC && b_kc == BKC && a2k == A2 && b2k == B2) {                                                      \
        if (bk == 16) rn_gemm_launch_one<128, 160, 4, 1, 16, AKC, BKC, false, A2, B2>(k, grid, st);                  \
        else rn_gemm_launch_one<128, 160, 4, 1, 32, AKC, BKC, false, A2, B2>(k, grid, st);                           \
        RN_LAUNCH_CHECK();                                                                                           \
        return RECNOW_OK;                                                                                            \
    }
    RN_GEMM_LEAN_LIST(X)
#undef X
    return RN_EINTERNAL;
}

// The instantiation lists of the GEMM kernels, one X(...) row per (layout, operand kind) combination.  Two readers: each gemm_inst_*.hip (and
// gemm_split.hip) expands its list into its launcher, and gemm_dispatch.hpp expands the same list into a host-only "is instantiated" predicate, so
// the plan names only kernels that exist and no launcher is ever tried.  No HIP in here.
#pragma once

// lean 128 x 128 and 128 x 160 (gemm_inst_lean128.hip, gemm_inst_lean160.hip), each at BK 16 and 32: X(A_KC, B_KC, A2K, B2K)
#define RN_GEMM_LEAN_LIST(X)   \
    X(true, false, 0, 0)       \
    X(true, false, 3, 0)       \
    X(true, true, 0, 0)        \
    X(true, true, 1, 0)        \
    X(true, true, 2, 0)        \
    X(true, true, 3, 0)        \
    X(false, false, 0, 0)      \
    X(false, false, 1, 0)      \
    X(false, false, 0, 2)      \
    X(false, false, 0, 3)

// lean 256 x 64 (gemm_inst_lean64.hip), BK 32: (B,S)x(S,S)-like products and CIN's N = F product.  X(A_KC, B_KC, A2K, B2K)
#define RN_GEMM_LEAN64_LIST(X)                                                                              \
    X(true, false, 3, 0) /* CIN: dx0t += (dX_k (x) X_{k-1}) W_k  (N = F <= 64) */                           \
    X(true, true, 0, 0)                                                                                     \
    X(true, false, 0, 0)

// lean 128 x 128 with a side product / rank-R update (gemm_inst_lean128x.hip), each at BK 16 and 32: X(A_KC, B_KC, A2K, B2K, XF)
#define RN_GEMM_LEAN128X_LIST(X)                                                                                                             \
    X(true, false, 0, 0, 1)   /* GEMM1:   x_l U           + gate logits as side product */                                                  \
    X(true, false, 0, 0, 9)   /*          ... XF | 8: at most two side columns (two experts), two-wide side product */                      \
    X(true, true, 1, 0, 9)                                                                                                                   \
    X(true, true, 0, 0, 9)                                                                                                                   \
    X(false, false, 0, 0, 9)                                                                                                                 \
    X(false, false, 1, 0, 9)                                                                                                                 \
    X(false, false, 0, 0, 41) /* XF | 32: both operands staged by LDS-DMA (RECNOW_GEMM_GLDS=1: the A/B of DESIGN 5k) */                      \
    X(false, true, 0, 0, 25)  /* GEMM1 transposed ([U | K]^T x_l^T) with the sub-space forward in its epilogue (XF | 16) */                  \
    X(false, true, 0, 1, 25)  /*          ... x_l = x0 * O_{l-1} formed in the operand load (dcnmix.hip mix_xless) */                        \
    X(true, false, 1, 0, 9)   /* GEMM1 (not transposed) of a layer l > 0 likewise */                                                        \
    X(true, false, 1, 0, 1)   /*          ... four-wide form (k-tiles of 16: D <= 256) */                                                   \
    X(true, false, 0, 0, 2)   /* GEMM3:   T2g W           + gate-weighted bias as rank-2 update */                                          \
    X(true, true, 1, 0, 1)    /* dT2g:    (x*g) W^T       + bias columns as side product */                                                 \
    X(true, true, 1, 0, 5)    /*          ... and dx = g * O written from the A stream (top layer) */                                       \
    X(true, true, 0, 0, 1)    /* dT2g of the top layer under a fused scoring head: x (W * w_head)^T, rows scaled by dscore later */         \
    X(true, true, 0, 0, 2)    /* dxl:     dA U^T          + dlogits K^T as rank-2 update */                                                 \
    X(false, false, 0, 0, 1)  /* dU:      x_l^T dA        + dgate as side product */                                                        \
    X(false, false, 1, 0, 1)  /* dW^T:    (x*g)^T T2g     + dbias as side product */

// lean 64 x 128 with the two-wide side product (gemm_inst_lean64x.hip), BK 32: X(A_KC, B_KC, A2K, B2K, XF)
#define RN_GEMM_LEAN64X_LIST(X)                                                                                              \
    X(true, false, 0, 0, 9)   /* GEMM1:  x_l [U | K] */                                                                      \
    X(true, false, 1, 0, 9)   /*         (x0 * O_{l-1}) [U | K]: x_l formed in the operand load (dcnmix.hip mix_xless) */    \
    X(true, true, 1, 0, 9)    /* dT2g:   (x * g) Wc2^T */                                                                    \
    X(true, true, 0, 0, 9)    /* dT2g of the top layer under the fused head */                                               \
    X(false, false, 0, 0, 9)  /* dU:     x_l^T dT1 */                                                                        \
    X(false, false, 1, 0, 9)  /* dW^T:   (x * g)^T T2g */

// k_gemm_split (gemm_split.hip): X(A_KC, A2K, BP), BP = where B comes from: 0 [k][n] rows, 1 [n][k] rows (both split in the kernel), 2 piece planes
#define RN_GEMM_SPLIT_LIST(X)                                                                       \
    X(true, 0, 0)     /* GEMM1:  x_l U */                                                           \
    X(true, 1, 1)     /* dT2g:   (x*g) W^T */                                                       \
    X(true, 0, 1)     /* dT2g of the top layer under a fused scoring head */                        \
    X(false, 0, 0)    /* dU:     x_l^T dA */                                                        \
    X(false, 1, 0)    /* dW^T:   (x*g)^T T2g */                                                     \
    X(true, 0, 2)     /* A [m][k] against B pre-split into planes (K <= 4096) */                    \
    X(true, 1, 2)

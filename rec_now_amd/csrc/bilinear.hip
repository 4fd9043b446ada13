// BilinearInteractionLayer (FiBiNET, Huang, Zhang and Zhang 2019, arXiv 1905.09433, section 3.3) -- C ABI 25.
//   out[b][p*D + d] = (x_i[b] W[w(p)])[d] * x_j[b][d]       pairs p = (i, j), i < j, in InnerPNN's i-major order
//   w(p) = 0 ('all'), i ('each'), p ('interaction');   W (nW, D, D) row-major, nW = 1 / F-1 / P.
// Same conventions as interact.hip: `fields` is a DEVICE array of F device pointers to contiguous (B, D) fp32 tensors, no float
// atomics, every reduction in a fixed order.  fp32 FMA on exact fp32 operands throughout; U = X W lives in LDS or registers only.
//
// Routes (recnow_bilinear_route):
//   ROW  ('all', 'each'): one wave per sample.  The sample's F x D block and U (F-1 x D) sit in wave-private LDS tiles, the weights
//         are resident in LDS for the whole launch where they fit (BIL_ROUTE_ROW_LDS) and read through L2 otherwise
//         (BIL_ROUTE_ROW_GLOBAL).  The output row leaves as one contiguous run of 16-byte stores.
//   TILE ('interaction'): a workgroup owns a tile of R samples and walks the pairs in batches of PB; the PB weight matrices of a batch
//         are staged in LDS once per tile, so W[p] is fetched once per R samples.
// Every LDS image has the row stride DP = 4 * ceil(D / 4), zero padded, so all LDS traffic is 16-byte; a global access is one
// 16-byte access when D % 4 == 0 and the tensor's base is 16-byte aligned, and up to four guarded 4-byte accesses otherwise (decided
// per tensor, in the kernel: the field pointers are device-resident).
//
// Backward workspace (recnow_bilinear_workspace_bytes; the carve order of recnow_bilinear_bwd):
//   [dU]    'all' / 'each' only:  B * (F-1) * D floats -- dU_i[b] = sum_j g_ij[b] * x_j[b], read back by the weight-gradient pass
//   [part]  G * S * D * D floats  -- per row-chunk partial sums of the weight gradient, S = F-1 ('all', 'each') or P ('interaction'),
//           G = rn_part_groups(B, BIL_DW_ROWS, BIL_DW_MAXG, S D^2) = max(1, min(ceil(B / BIL_DW_ROWS), BIL_DW_MAXG, RN_PART_BYTES / (4 S D^2)))
//   each carve rounded up to 256 bytes.  Nothing grows as B * P * D^2.
#include "common.hpp"
#include "partials.hpp"

#define BIL_ALL 0
#define BIL_EACH 1
#define BIL_INTER 2
#define BIL_ROUTE_ROW_LDS 0
#define BIL_ROUTE_ROW_GLOBAL 1
#define BIL_ROUTE_TILE 2
#define BIL_MAX_F 64
#define BIL_MAX_D 64
#define BIL_LDS_BYTES (64 * 1024)
#define BIL_W_STAGE_FLOATS 4096                 // LDS floats of one staged batch of weight matrices (TILE routes)
#define BIL_TILE_X_FLOATS 10240                 // LDS floats of the X tile of the TILE forward
#define BIL_TILE_DX_FLOATS 8192                 // LDS floats of the dX accumulators of the TILE backward
#define BIL_TILE_MAX_ROWS 64
#define BIL_BWD_PB 12                           // pairs of one staged batch of the TILE backward at the most (their g, x_j sit in registers)
#define BIL_ROW_GRID 2048
#define BIL_TILE_GRID 2048
#define BIL_DW_ROWS 256                         // rows of one weight-gradient partial at the least
#define BIL_DW_MAXG 256

// e / Qp for e * Qp < 2^32 (magic = 2^32 / Qp + 1; Qp == 1 has no 32-bit magic)
__device__ __forceinline__ int bil_div(int e, int Qp, unsigned magic) { return Qp == 1 ? e : (int)__umulhi((unsigned)e, magic); }
__device__ __forceinline__ int bil_pair(int i, int j, int F) { return i * F - i * (i + 1) / 2 + (j - i - 1); }
// pair table: pt[p] = i | j << 8
__device__ __forceinline__ void bil_fill_pairs(unsigned short* pt, int F, int P) {
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        int i = 0;
        while (bil_pair(i + 1, i + 2, F) <= p && i + 2 < F) ++i;
        pt[p] = (unsigned short)(i | ((i + 1 + p - bil_pair(i, i + 1, F)) << 8));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// ROW routes.  LDS: [wl: nWl * D * DP, resident weights (wres)] [pt: P shorts] [per wave: xs, us (, dus): F * DP each]
// ---------------------------------------------------------------------------------------------------------------------
struct BilRow {
    int F, D, Qp, DP, P, type, wres, ptf;       // ptf: floats of the pair table
    unsigned magic;
    int64_t B;
};
// stage the resident weights and the pair table (whole workgroup)
__device__ __forceinline__ void bil_row_prologue(const BilRow& c, const float* W, float* wl, unsigned short* pt) {
    if (c.wres) {
        const int nW = c.type == BIL_ALL ? 1 : c.F - 1;
        const bool vw = rn_vec4_ok(W, c.D);
        for (int e = threadIdx.x; e < nW * c.D * c.Qp; e += blockDim.x) {
            const int row = e / c.Qp, q = e - row * c.Qp;
            *reinterpret_cast<rn_f4*>(wl + row * c.DP + 4 * q) = rn_ld4(W + (int64_t)row * c.D + 4 * q, c.D - 4 * q, vw);
        }
    }
    bil_fill_pairs(pt, c.F, c.P);
    __syncthreads();
}
// the sample's X block -> xs, then U_i = x_i W[w(i)] -> us (one wave)
__device__ __forceinline__ void bil_row_xu(const BilRow& c, const float* const* fields, const float* W, const float* wl, float* xs, float* us,
                                           int64_t b, int lane) {
    for (int e = lane; e < c.F * c.Qp; e += 64) {
        const int f = bil_div(e, c.Qp, c.magic), q = e - f * c.Qp;
        const float* xf = fields[f];
        *reinterpret_cast<rn_f4*>(xs + f * c.DP + 4 * q) = rn_ld4(xf + b * c.D + 4 * q, c.D - 4 * q, rn_vec4_ok(xf, c.D));
    }
    RN_LDS_WAVE_SYNC();
    const bool vw = rn_vec4_ok(W, c.D);
    for (int e = lane; e < (c.F - 1) * c.Qp; e += 64) {
        const int i = bil_div(e, c.Qp, c.magic), q = e - i * c.Qp;
        const int wi = c.type == BIL_ALL ? 0 : i;
        rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c.wres) {
            const float* wr = wl + wi * c.D * c.DP + 4 * q;
            for (int k = 0; k < c.D; ++k) acc += xs[i * c.DP + k] * *reinterpret_cast<const rn_f4*>(wr + k * c.DP);
        } else {
            const float* wr = W + (int64_t)wi * c.D * c.D + 4 * q;
            for (int k = 0; k < c.D; ++k) acc += xs[i * c.DP + k] * rn_ld4(wr + k * c.D, c.D - 4 * q, vw);
        }
        *reinterpret_cast<rn_f4*>(us + i * c.DP + 4 * q) = acc;
    }
    RN_LDS_WAVE_SYNC();
}

__global__ void __launch_bounds__(256)
k_bil_row_fwd(const float* const* __restrict__ fields, const float* __restrict__ W, float* __restrict__ out, BilRow c) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nWl = c.wres ? (c.type == BIL_ALL ? 1 : c.F - 1) : 0;
    float* wl = bil_lds;
    unsigned short* pt = reinterpret_cast<unsigned short*>(wl + nWl * c.D * c.DP);
    float* xs = wl + nWl * c.D * c.DP + c.ptf + w * 2 * c.F * c.DP;
    float* us = xs + c.F * c.DP;
    bil_row_prologue(c, W, wl, pt);
    const bool vo = rn_vec4_ok(out, c.D);
    const int E = c.P * c.Qp;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < c.B; b += (int64_t)gridDim.x * nw) {
        bil_row_xu(c, fields, W, wl, xs, us, b, lane);
        float* ob = out + b * c.P * c.D;
        for (int e = lane; e < E; e += 64) {
            const int p = bil_div(e, c.Qp, c.magic), q = e - p * c.Qp;
            const int ij = pt[p], i = ij & 255, j = ij >> 8;
            const rn_f4 o = *reinterpret_cast<const rn_f4*>(us + i * c.DP + 4 * q) * *reinterpret_cast<const rn_f4*>(xs + j * c.DP + 4 * q);
            rn_st4_stream(ob + p * c.D + 4 * q, o, c.D - 4 * q, vo);
        }
        RN_LDS_WAVE_SYNC();                                    // tiles read before the next sample overwrites them
    }
}

// One pass over the sample's dout row (each g_ij is fetched for dU_i and, from L2, for dX_j):
//   dU_f = sum_{j > f} g_fj * x_j          -> dus (and the workspace when the weight gradient is wanted)
//   dX_f = sum_{i < f} g_if * U_i + dU_f W[w(f)]^T
__global__ void __launch_bounds__(256)
k_bil_row_bwd(const float* const* __restrict__ fields, float* const* __restrict__ dfields, const float* __restrict__ W,
              const float* __restrict__ dout, float* __restrict__ du_ws, BilRow c) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nWl = c.wres ? (c.type == BIL_ALL ? 1 : c.F - 1) : 0;
    float* wl = bil_lds;
    unsigned short* pt = reinterpret_cast<unsigned short*>(wl + nWl * c.D * c.DP);
    float* xs = wl + nWl * c.D * c.DP + c.ptf + w * 3 * c.F * c.DP;
    float* us = xs + c.F * c.DP;
    float* dus = us + c.F * c.DP;
    bil_row_prologue(c, W, wl, pt);
    const bool vg = rn_vec4_ok(dout, c.D), vw = rn_vec4_ok(W, c.D), vu = rn_vec4_ok(du_ws, c.D);
    const int F = c.F, D = c.D, DP = c.DP;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < c.B; b += (int64_t)gridDim.x * nw) {
        bil_row_xu(c, fields, W, wl, xs, us, b, lane);
        const float* gb = dout + b * c.P * D;
        for (int e = lane; e < F * c.Qp; e += 64) {
            const int f = bil_div(e, c.Qp, c.magic), q = e - f * c.Qp;
            rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
            const float* gr = gb + (int64_t)bil_pair(f, f + 1, F) * D + 4 * q;      // the run of pairs (f, f+1 ..): only read for f < F-1
#pragma unroll 4
            for (int j = f + 1; j < F; ++j) acc += rn_ld4(gr + (j - f - 1) * D, D - 4 * q, vg) * *reinterpret_cast<const rn_f4*>(xs + j * DP + 4 * q);
            *reinterpret_cast<rn_f4*>(dus + f * DP + 4 * q) = acc;
            if (du_ws && f < F - 1) rn_st4(du_ws + (b * (F - 1) + f) * D + 4 * q, acc, D - 4 * q, vu);
        }
        RN_LDS_WAVE_SYNC();
        for (int e = lane; e < F * c.Qp; e += 64) {
            const int f = bil_div(e, c.Qp, c.magic), q = e - f * c.Qp;
            rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int i = 0; i < f; ++i)
                acc += rn_ld4(gb + (int64_t)bil_pair(i, f, F) * D + 4 * q, D - 4 * q, vg) * *reinterpret_cast<const rn_f4*>(us + i * DP + 4 * q);
            if (f < F - 1) {
                const int wi = c.type == BIL_ALL ? 0 : f;
                float r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = 4 * q + t;
                    if (k < D) {
                        rn_f4 s = {0.f, 0.f, 0.f, 0.f};
                        if (c.wres) {
                            const float* wr = wl + (wi * D + k) * DP;
                            for (int d = 0; d < DP; d += 4) s += *reinterpret_cast<const rn_f4*>(dus + f * DP + d) * *reinterpret_cast<const rn_f4*>(wr + d);
                        } else {
                            const float* wr = W + ((int64_t)wi * D + k) * D;
                            for (int d = 0; d < DP; d += 4) s += *reinterpret_cast<const rn_f4*>(dus + f * DP + d) * rn_ld4(wr + d, D - d, vw);
                        }
                        r[t] = (s.x + s.y) + (s.z + s.w);
                    }
                }
                acc += rn_f4{r[0], r[1], r[2], r[3]};
            }
            float* df = dfields[f];
            rn_st4(df + b * D + 4 * q, acc, D - 4 * q, rn_vec4_ok(df, D));
        }
        RN_LDS_WAVE_SYNC();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// TILE routes ('interaction').
// ---------------------------------------------------------------------------------------------------------------------
struct BilTile {
    int F, D, Qp, DP, P, R, PB, lpr_shift, ptf;        // lpr_shift: log2 of the lanes that serve one row
    unsigned magic;
    int64_t B;
};
// the PBc weight matrices from pair p0 on -> wt[pp][k][ws], ws >= DP the row stride
__device__ __forceinline__ void bil_stage_w(const BilTile& c, const float* W, float* wt, int p0, int PBc, int ws) {
    const bool vw = rn_vec4_ok(W, c.D);
    for (int e = threadIdx.x; e < PBc * c.D * c.Qp; e += blockDim.x) {
        const int row = e / c.Qp, q = e - row * c.Qp;
        *reinterpret_cast<rn_f4*>(wt + row * ws + 4 * q) = rn_ld4(W + ((int64_t)p0 * c.D + row) * c.D + 4 * q, c.D - 4 * q, vw);
    }
}

// LDS: [xt: R * F * DP] [wt: PB * D * DP] [pt].  Thread (rr, cc): rows rr, rr + 256/LPR, ..; (pair, float4) items cc, cc + LPR, .. of a batch:
// consecutive lanes write consecutive 16-byte pieces of one output row.
__global__ void __launch_bounds__(256)
k_bil_tile_fwd(const float* const* __restrict__ fields, const float* __restrict__ W, float* __restrict__ out, BilTile c) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    float* xt = bil_lds;
    float* wt = xt + c.R * c.F * c.DP;
    unsigned short* pt = reinterpret_cast<unsigned short*>(wt + c.PB * c.D * c.DP);
    bil_fill_pairs(pt, c.F, c.P);
    const int F = c.F, D = c.D, DP = c.DP, Qp = c.Qp;
    const int LPR = 1 << c.lpr_shift, rr = threadIdx.x >> c.lpr_shift, cc = threadIdx.x & (LPR - 1), rstep = 256 >> c.lpr_shift;
    const bool vo = rn_vec4_ok(out, D);
    const int64_t ntiles = (c.B + c.R - 1) / c.R;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * c.R;
        const int rows = (int)min((int64_t)c.R, c.B - b0);
        __syncthreads();                                    // the previous tile is consumed
        for (int f = 0; f < F; ++f) {                       // the field's rows x D block is contiguous in its tensor
            const float* xf = fields[f];
            const bool vx = rn_vec4_ok(xf, D);
            for (int e = threadIdx.x; e < rows * Qp; e += 256) {
                const int r = bil_div(e, Qp, c.magic), q = e - r * Qp;
                *reinterpret_cast<rn_f4*>(xt + (r * F + f) * DP + 4 * q) = rn_ld4(xf + (b0 + r) * D + 4 * q, D - 4 * q, vx);
            }
        }
        for (int p0 = 0; p0 < c.P; p0 += c.PB) {
            const int PBc = min(c.PB, c.P - p0);
            __syncthreads();                                // X tile written / previous batch consumed
            bil_stage_w(c, W, wt, p0, PBc, DP);
            __syncthreads();
            for (int r = rr; r < rows; r += 4 * rstep) {     // rows r, r + rstep, .. (4 of them) share every weight read
                int rk[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) rk[t] = min(r + t * rstep, rows - 1);       // past the tile: recomputes the last row, stores nothing
                for (int c2 = cc; c2 < PBc * Qp; c2 += LPR) {
                    const int pp = bil_div(c2, Qp, c.magic), q = c2 - pp * Qp;
                    const int ij = pt[p0 + pp], i = ij & 255, j = ij >> 8;
                    const float* wr = wt + pp * D * DP + 4 * q;
                    rn_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
                    for (int k = 0; k < D; k += 4) {
                        const rn_f4 x0 = *reinterpret_cast<const rn_f4*>(xt + (rk[0] * F + i) * DP + k);
                        const rn_f4 x1 = *reinterpret_cast<const rn_f4*>(xt + (rk[1] * F + i) * DP + k);
                        const rn_f4 x2 = *reinterpret_cast<const rn_f4*>(xt + (rk[2] * F + i) * DP + k);
                        const rn_f4 x3 = *reinterpret_cast<const rn_f4*>(xt + (rk[3] * F + i) * DP + k);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            if (k + t < D) {                 // rows k >= D of the staged matrix belong to the next pair
                                const rn_f4 w4 = *reinterpret_cast<const rn_f4*>(wr + (k + t) * DP);
                                a0 += x0[t] * w4; a1 += x1[t] * w4; a2 += x2[t] * w4; a3 += x3[t] * w4;
                            }
                        }
                    }
                    const rn_f4 acc[4] = {a0, a1, a2, a3};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (r + t * rstep < rows) {
                            const rn_f4 o = acc[t] * *reinterpret_cast<const rn_f4*>(xt + (rk[t] * F + j) * DP + 4 * q);
                            rn_st4_stream(out + ((b0 + rk[t]) * c.P + (p0 + pp)) * D + 4 * q, o, D - 4 * q, vo);
                        }
                    }
                }
            }
        }
    }
}

// LDS: [dxt: R rows of F * DP + 4 accumulators] [wt: PB * D rows of DP + 4] [xi: R rows of DP + 4] [ht: the same].  The strides are padded
// by one 16-byte slot: the lanes of a wave differ in the row r, and unpadded rows of 16 .. 64 floats put them on the same banks.
// Thread (r, q) = (tid / LPR, tid % LPR), LPR a power of two >= Qp so that the lanes of a row share a wave.  The thread streams its row's
// dout over all pairs in order, a batch's g and x_j pieces requested together; every LDS accumulator slot
// (r, f, q) belongs to one thread, so the sums have one fixed order.
//   U_p[4q..] = x_i W[p][:, 4q..];  dX_j[4q..] += g * U_p;  h = g * x_j -> ht;  dX_i[4q + t] += <h, W[p][4q + t][:]>
__global__ void __launch_bounds__(256)
k_bil_tile_bwd(const float* const* __restrict__ fields, float* const* __restrict__ dfields, const float* __restrict__ W,
               const float* __restrict__ dout, BilTile c) {
    extern __shared__ __attribute__((aligned(16))) float bil_lds[];
    const int F = c.F, D = c.D, DP = c.DP, Qp = c.Qp;
    const int XS = DP + 4, RS = F * DP + 4;
    float* dxt = bil_lds;
    float* wt = dxt + c.R * RS;
    float* xi = wt + c.PB * D * XS;
    float* ht = xi + c.R * XS;
    const int LPR = 1 << c.lpr_shift, r = threadIdx.x >> c.lpr_shift, q = threadIdx.x & (LPR - 1);
    const bool vg = rn_vec4_ok(dout, D);
    int kt[4];                                              // the rows of W[p] this thread contracts h with, clamped into the matrix
#pragma unroll
    for (int t = 0; t < 4; ++t) kt[t] = min(4 * q + t, D - 1);
    const int64_t ntiles = (c.B + c.R - 1) / c.R;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b0 = tile * c.R;
        const int rows = (int)min((int64_t)c.R, c.B - b0);
        const bool active = r < rows && q < Qp;
        const int64_t b = b0 + (active ? r : 0);
        float* dxr = dxt + (active ? r : 0) * RS + 4 * q;
        if (active)
            for (int f = 0; f < F; ++f) *reinterpret_cast<rn_f4*>(dxr + f * DP) = rn_f4{0.f, 0.f, 0.f, 0.f};
        const float* gb = dout + b * c.P * D + 4 * q;
        int i = 0, j = 0, icur = -1;                        // (i, j) of pair p, advanced in step with p
        rn_f4 dxi = {0.f, 0.f, 0.f, 0.f};
        for (int p0 = 0; p0 < c.P; p0 += c.PB) {
            const int PBc = min(c.PB, c.P - p0);
            // the batch's g and x_j pieces of this thread, all requested at once and ahead of the weight staging: BIL_BWD_PB independent
            // loads in flight per lane instead of one (few waves fit beside the LDS accumulators, so the loads must overlap inside a thread)
            rn_f4 gq[BIL_BWD_PB], xq[BIL_BWD_PB];
            {
                int i2 = i, j2 = j;
#pragma unroll
                for (int pp = 0; pp < BIL_BWD_PB; ++pp) {
                    gq[pp] = rn_f4{0.f, 0.f, 0.f, 0.f};
                    xq[pp] = gq[pp];
                    if (pp < PBc) {
                        if (++j2 >= F) { ++i2; j2 = i2 + 1; }
                        if (active) {
                            const float* xf = fields[j2];
                            xq[pp] = rn_ld4(xf + b * D + 4 * q, D - 4 * q, rn_vec4_ok(xf, D));
                            gq[pp] = rn_ld4(gb + (int64_t)(p0 + pp) * D, D - 4 * q, vg);
                        }
                    }
                }
            }
            __syncthreads();                                // previous batch consumed
            bil_stage_w(c, W, wt, p0, PBc, XS);
            __syncthreads();
            // one pair; called with constant indices below so that gq / xq stay in registers
            auto step = [&](const int pp, const rn_f4 g, const rn_f4 xj) __attribute__((always_inline)) {
                if (++j >= F) { ++i; j = i + 1; }
                if (i != icur) {                            // uniform over the workgroup
                    if (active && icur >= 0) *reinterpret_cast<rn_f4*>(dxr + icur * DP) += dxi;
                    dxi = rn_f4{0.f, 0.f, 0.f, 0.f};
                    icur = i;
                    RN_LDS_WAVE_SYNC();                        // the row's lanes have read the previous x_i
                    if (active) {
                        const float* xf = fields[i];
                        *reinterpret_cast<rn_f4*>(xi + r * XS + 4 * q) = rn_ld4(xf + b * D + 4 * q, D - 4 * q, rn_vec4_ok(xf, D));
                    }
                    RN_LDS_WAVE_SYNC();
                }
                const float* wr = wt + pp * D * XS;
                if (active) {
                    rn_f4 u = {0.f, 0.f, 0.f, 0.f};
                    for (int k = 0; k < D; k += 4) {
                        const rn_f4 x4 = *reinterpret_cast<const rn_f4*>(xi + r * XS + k);
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (k + t < D) u += x4[t] * *reinterpret_cast<const rn_f4*>(wr + (k + t) * XS + 4 * q);
                    }
                    *reinterpret_cast<rn_f4*>(dxr + j * DP) += g * u;
                    *reinterpret_cast<rn_f4*>(ht + r * XS + 4 * q) = g * xj;
                }
                RN_LDS_WAVE_SYNC();
                if (active) {
                    rn_f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
                    for (int d = 0; d < DP; d += 4) {       // h is zero past D: the padded columns of wt add nothing
                        const rn_f4 h4 = *reinterpret_cast<const rn_f4*>(ht + r * XS + d);
                        s0 += h4 * *reinterpret_cast<const rn_f4*>(wr + kt[0] * XS + d);
                        s1 += h4 * *reinterpret_cast<const rn_f4*>(wr + kt[1] * XS + d);
                        s2 += h4 * *reinterpret_cast<const rn_f4*>(wr + kt[2] * XS + d);
                        s3 += h4 * *reinterpret_cast<const rn_f4*>(wr + kt[3] * XS + d);
                    }
                    // components 4q + t >= D repeat row D-1: never stored
                    dxi += rn_f4{(s0.x + s0.y) + (s0.z + s0.w), (s1.x + s1.y) + (s1.z + s1.w), (s2.x + s2.y) + (s2.z + s2.w), (s3.x + s3.y) + (s3.z + s3.w)};
                }
                RN_LDS_WAVE_SYNC();                            // ht read before the next pair overwrites it
            };
#define BIL_STEP(PP) if (PP < PBc) step(PP, gq[PP], xq[PP])
            BIL_STEP(0); BIL_STEP(1); BIL_STEP(2); BIL_STEP(3); BIL_STEP(4); BIL_STEP(5);
            BIL_STEP(6); BIL_STEP(7); BIL_STEP(8); BIL_STEP(9); BIL_STEP(10); BIL_STEP(11);
#undef BIL_STEP
            static_assert(BIL_BWD_PB == 12, "one BIL_STEP per pair of a batch");
        }
        if (active) {
            if (icur >= 0) *reinterpret_cast<rn_f4*>(dxr + icur * DP) += dxi;
            for (int f = 0; f < F; ++f) {
                float* df = dfields[f];
                rn_st4(df + b * D + 4 * q, *reinterpret_cast<const rn_f4*>(dxr + f * DP), D - 4 * q, rn_vec4_ok(df, D));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient: dW[w(s)][k][d] = sum_b x_{i(s)}[b][k] * h_s[b][d] over the slots s; h_s = dU_s from the workspace ('all', 'each',
// slot = field i) or g_s * x_{j(s)} formed on the fly ('interaction', slot = pair).  Workgroup (slot chunk, row chunk); a thread owns the
// 4 x 4 block (k quad, d quad) of one slot and sums its row chunk in row order in fp32; rn_part_reduce (partials.hpp) adds the row chunks (and
// for 'all' the slots, slot-major) in fp64 in a fixed tree.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_bil_dw_partial(const float* const* __restrict__ fields, const float* __restrict__ dout, const float* __restrict__ du_ws,
                 float* __restrict__ part, int F, int D, int Qp, int P, int type, int S, int SB, int64_t B, int64_t rows_per_g) {
    const int it = threadIdx.x;
    const int ss = it / (Qp * Qp), rem = it - ss * Qp * Qp, kq = rem / Qp, q = rem - kq * Qp;
    const int s = blockIdx.x * SB + ss;
    if (ss >= SB || s >= S) return;                         // no barrier in this kernel
    int i = s, j = 0;
    if (type == BIL_INTER) {
        i = 0;
        while (bil_pair(i + 1, i + 2, F) <= s && i + 2 < F) ++i;
        j = i + 1 + s - bil_pair(i, i + 1, F);
    }
    const float* xi = fields[i];
    const float* xj = fields[j];
    const bool vi = rn_vec4_ok(xi, D), vj = rn_vec4_ok(xj, D), vg = rn_vec4_ok(dout, D), vu = rn_vec4_ok(du_ws, D);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_g, r1 = min(B, r0 + rows_per_g);
    rn_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 2
    for (int64_t b = r0; b < r1; ++b) {
        const rn_f4 x = rn_ld4(xi + b * D + 4 * kq, D - 4 * kq, vi);
        rn_f4 h;
        if (type == BIL_INTER) h = rn_ld4(dout + (b * P + s) * D + 4 * q, D - 4 * q, vg) * rn_ld4(xj + b * D + 4 * q, D - 4 * q, vj);
        else h = rn_ld4(du_ws + (b * (F - 1) + s) * D + 4 * q, D - 4 * q, vu);
        a0 += x.x * h; a1 += x.y * h; a2 += x.z * h; a3 += x.w * h;
    }
    float* o = part + ((int64_t)blockIdx.y * S + s) * D * D;
    const rn_f4 acc[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = 4 * kq + t;
        if (k < D) rn_st4(o + k * D + 4 * q, acc[t], D - 4 * q, rn_vec4_ok(part, D));
    }
}
// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
static inline bool bil_shape_ok(int F, int D, int type) { return F >= 1 && F <= BIL_MAX_F && D >= 1 && D <= BIL_MAX_D && type >= BIL_ALL && type <= BIL_INTER; }
static inline unsigned bil_magic(int Qp) { return Qp == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)Qp + 1); }
static inline int bil_ptf(int P) { return ((P + 1) / 2 + 3) & ~3; }

// waves per workgroup, weight residency and LDS bytes of a ROW kernel with `ntile` wave-private F x DP tiles
static void bil_row_cfg(int F, int D, int type, int ntile, int* waves, int* wres, size_t* lds) {
    const int DP = (D + 3) & ~3, P = F * (F - 1) / 2;
    const size_t wfl = (size_t)(type == BIL_ALL ? 1 : F - 1) * D * DP, tile = (size_t)F * DP;
    static const int order[6][2] = {{4, 1}, {2, 1}, {4, 0}, {2, 0}, {1, 1}, {1, 0}};
    for (int t = 0; t < 6; ++t) {
        const size_t bytes = 4 * ((order[t][1] ? wfl : 0) + bil_ptf(P) + (size_t)order[t][0] * ntile * tile);
        if (bytes <= BIL_LDS_BYTES || t == 5) {             // the last entry always fits: 3 * 64 * 64 + 1008 floats
            *waves = order[t][0];
            *wres = order[t][1];
            *lds = bytes;
            return;
        }
    }
}
static BilRow bil_row_desc(int F, int D, int type, int wres, int64_t B) {
    BilRow c;
    c.F = F; c.D = D; c.Qp = (D + 3) / 4; c.DP = 4 * c.Qp; c.P = F * (F - 1) / 2; c.type = type; c.wres = wres; c.ptf = bil_ptf(c.P);
    c.magic = bil_magic(c.Qp); c.B = B;
    return c;
}
static BilTile bil_tile_desc(int F, int D, int64_t B, bool bwd, size_t* lds, int* threads) {
    BilTile c;
    c.F = F; c.D = D; c.Qp = (D + 3) / 4; c.DP = 4 * c.Qp; c.P = F * (F - 1) / 2; c.ptf = bil_ptf(c.P); c.magic = bil_magic(c.Qp); c.B = B;
    c.PB = BIL_W_STAGE_FLOATS / (D * (bwd ? c.DP + 4 : c.DP));
    if (c.PB < 1) c.PB = 1;
    if (c.PB > c.P) c.PB = c.P;
    if (bwd && c.PB > BIL_BWD_PB) c.PB = BIL_BWD_PB;
    if (!bwd) {
        c.R = BIL_TILE_X_FLOATS / (F * c.DP);
        if (c.R < 1) c.R = 1;
        if (c.R > BIL_TILE_MAX_ROWS) c.R = BIL_TILE_MAX_ROWS;
        int sh = 0;
        while ((1 << sh) < c.PB * c.Qp && sh < 8) ++sh;      // lanes per row: the batch's float4 items, at most the workgroup
        c.lpr_shift = sh;
        *lds = 4 * ((size_t)c.R * F * c.DP + (size_t)c.PB * D * c.DP + c.ptf);
        *threads = 256;
    } else {
        int sh = 0;
        while ((1 << sh) < c.Qp) ++sh;                       // lanes per row: a power of two >= Qp (<= 16)
        c.lpr_shift = sh;
        c.R = BIL_TILE_DX_FLOATS / (F * c.DP);
        if (c.R < 1) c.R = 1;
        if (c.R > (256 >> sh)) c.R = 256 >> sh;
        for (;;) {                                           // rows of F * DP + 4, weight rows and x_i / h rows of DP + 4 floats
            *lds = 4 * ((size_t)c.R * (F * c.DP + 4) + (size_t)c.PB * D * (c.DP + 4) + 2 * (size_t)c.R * (c.DP + 4));
            if (*lds <= BIL_LDS_BYTES || c.R == 1) break;
            --c.R;
        }
        *threads = ((c.R << sh) + 63) & ~63;
    }
    return c;
}
// slots and row chunks of the weight-gradient partials
static void bil_dw_cfg(int64_t B, int F, int D, int type, int* S, int* G) {
    *S = type == BIL_INTER ? F * (F - 1) / 2 : F - 1;
    *G = rn_part_groups(B, BIL_DW_ROWS, BIL_DW_MAXG, (int64_t)*S * D * D);
}

extern "C" int recnow_bilinear_supported(int F, int D, int type) { return bil_shape_ok(F, D, type) ? 1 : 0; }

extern "C" int recnow_bilinear_route(int F, int D, int type, int bwd) {
    if (!bil_shape_ok(F, D, type)) return RECNOW_EUNSUPPORTED;
    if (type == BIL_INTER) return BIL_ROUTE_TILE;
    int waves, wres;
    size_t lds;
    bil_row_cfg(F, D, type, bwd ? 3 : 2, &waves, &wres, &lds);
    return wres ? BIL_ROUTE_ROW_LDS : BIL_ROUTE_ROW_GLOBAL;
}

extern "C" size_t recnow_bilinear_workspace_bytes(int64_t B, int F, int D, int type) {
    if (!bil_shape_ok(F, D, type) || B <= 0 || F < 2) return 0;
    int S, G;
    bil_dw_cfg(B, F, D, type, &S, &G);
    size_t bytes = rn_align((size_t)G * S * D * D * sizeof(float));
    if (type != BIL_INTER) bytes += rn_align((size_t)B * (F - 1) * D * sizeof(float));
    return bytes;
}

extern "C" int recnow_bilinear_fwd(const float* const* fields, int F, int64_t B, int D, int type, const float* W, float* out, void* stream) {
    if (F < 1 || B < 0 || D < 1 || type < BIL_ALL || type > BIL_INTER) return RECNOW_EINVAL;
    if (!bil_shape_ok(F, D, type)) return RECNOW_EUNSUPPORTED;
    if (B == 0 || F == 1) return RECNOW_OK;
    if (!fields || !W || !out) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (type == BIL_INTER) {
        size_t lds;
        int threads;
        const BilTile c = bil_tile_desc(F, D, B, false, &lds, &threads);
        int64_t g = (B + c.R - 1) / c.R;
        if (g > BIL_TILE_GRID) g = BIL_TILE_GRID;
        hipLaunchKernelGGL(k_bil_tile_fwd, (int)g, threads, lds, st, fields, W, out, c);
    } else {
        int waves, wres;
        size_t lds;
        bil_row_cfg(F, D, type, 2, &waves, &wres, &lds);
        int64_t g = (B + waves - 1) / waves;
        if (g > BIL_ROW_GRID) g = BIL_ROW_GRID;
        hipLaunchKernelGGL(k_bil_row_fwd, (int)g, waves * 64, lds, st, fields, W, out, bil_row_desc(F, D, type, wres, B));
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_bilinear_bwd(const float* const* fields, float* const* dfields, int F, int64_t B, int D, int type, const float* W,
                                   const float* dout, float* dW, void* ws, size_t ws_bytes, void* stream) {
    if (F < 1 || B < 0 || D < 1 || type < BIL_ALL || type > BIL_INTER) return RECNOW_EINVAL;
    if (!bil_shape_ok(F, D, type)) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!fields || !dfields || !W || (F > 1 && !dout)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* du = nullptr;
    float* part = nullptr;
    int S = 0, G = 0;
    if (dW && F > 1) {
        if (!ws || ws_bytes < recnow_bilinear_workspace_bytes(B, F, D, type)) return RECNOW_EWORKSPACE;
        bil_dw_cfg(B, F, D, type, &S, &G);
        RnCarver cv(ws, ws_bytes);
        if (type != BIL_INTER) du = cv.take<float>((size_t)B * (F - 1) * D);
        part = cv.take<float>((size_t)G * S * D * D);
        if (!cv.ok()) return RECNOW_EWORKSPACE;
    }
    if (type == BIL_INTER && F > 1) {
        size_t lds;
        int threads;
        const BilTile c = bil_tile_desc(F, D, B, true, &lds, &threads);
        int64_t g = (B + c.R - 1) / c.R;
        if (g > BIL_TILE_GRID) g = BIL_TILE_GRID;
        hipLaunchKernelGGL(k_bil_tile_bwd, (int)g, threads, lds, st, fields, dfields, W, dout, c);
    } else {
        // F == 1: no pair, dX_0 = 0 -- the ROW kernel writes it (its loops over pairs are empty)
        int waves, wres;
        size_t lds;
        bil_row_cfg(F, D, type == BIL_INTER ? BIL_ALL : type, 3, &waves, &wres, &lds);
        int64_t g = (B + waves - 1) / waves;
        if (g > BIL_ROW_GRID) g = BIL_ROW_GRID;
        hipLaunchKernelGGL(k_bil_row_bwd, (int)g, waves * 64, lds, st, fields, dfields, W, dout, du,
                           bil_row_desc(F, D, type == BIL_INTER ? BIL_ALL : type, F > 1 ? wres : 0, B));
    }
    RN_LAUNCH_CHECK();
    if (part) {
        const int Qp = (D + 3) / 4;
        int SB = 256 / (Qp * Qp);                            // slots of one workgroup: a 4 x 4 block per thread
        if (SB > S) SB = S;
        const int64_t rows_per_g = (B + G - 1) / G;
        hipLaunchKernelGGL(k_bil_dw_partial, dim3((S + SB - 1) / SB, G), 256, 0, st, fields, dout, du, part, F, D, Qp, F * (F - 1) / 2, type, S, SB,
                           B, rows_per_g);
        RN_LAUNCH_CHECK();
        // 'all': the S slots of a chunk are terms of one matrix, slot-major; else the slot is part of the element index
        const int64_t DD = (int64_t)D * D, n = type == BIL_ALL ? DD : S * DD;
        const RnPartDst dst = {{dW, nullptr, nullptr, nullptr}, {n, n, n, n}};
        return rn_part_reduce(part, n, type == BIL_ALL ? S : 1, G, S * DD, DD, dst, st);
    }
    return RECNOW_OK;
}

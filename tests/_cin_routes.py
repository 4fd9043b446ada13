"""The route table of CINLayer (csrc/cin.hip recnow_cin_fwd / recnow_cin_bwd, csrc/cin_bwd.hip): one row per distinct path through the two entry
points, with the call that reaches it.  Used by tests/test_cin_routes_gpu.py (on the GPU) and tests/test_cin_census_cpu.py (the census of every
row is exact and has teeth).

How a call picks its kernels:
  forward, layer k       one OUTER-operand product X_k (M x H_k) = Z (M x F H_{k-1}) W_k^T, M = B D, on the tile family of pick_cfg(H_k)
                         (csrc/gemm_dispatch.hpp): H_k <= 32: 256 x 32; <= 64: 256 x 64; 128 < H_k <= 160: 128 x 160; else 128 x 128.  M, H_k or
                         F H_{k-1} off the tile, or a misaligned operand: the edge kernel of the same family
  backward, layer k      dW_k = dX_k^T Z always (one product, K = M).  The data gradients: rn_cin_bwd_fused_ok -- M % 128 == 0, H_k % 32 == 0,
                         H_{k-1} in {64, 128}, F % 4 == 0, F H_{k-1} % 128 == 0, cb_lds_bytes(F) <= 160 KiB (F <= 92), and dX_k, W_k, x0t and both
                         outputs 16-byte aligned -- one k_cin_bwd_fused<H_{k-1}> launch (no profiler hook); else two more products (the second
                         behind k_cin_wt).  Layer 1 (H_0 = F = 64): both gradients land in dx0t (`same`)
  glue                   k_cin_in / _bwd, k_rowsum, k_fill_rowbcast, k_cin_concat / _bwd, k_cin_wt: ew_grid caps the grid at 8192 blocks of 256
                         (k_rowsum: 4 rows per block), beyond that the kernels stride

Row fields: name, B, D, F, Hs, modes ((output_input, sum_channel) pairs the row runs in), fused (per layer, 0-based: the fused kernel takes it),
tags (recnow_prof tags of the L forward products), census ((k, xmax, rho) of tests/_cin_census.py LADDER), why."""

T128, T160, T256x64, T256x32 = 1, 2, 3, 4                   # csrc/prof.hpp RN_TAG_GEMM_*
CB_BM, CB_BK, CB_LDA, CB_LDB = 128, 32, 129, 128            # csrc/cin_bwd.hip
_TAG = {(128, 128): T128, (128, 160): T160, (256, 64): T256x64, (256, 32): T256x32}


def pick_cfg(N):
    """csrc/gemm_dispatch.hpp pick_cfg(int N): the tile family (BM, BN) of a product with N output columns (no side product: never 64 x 128)"""
    if N <= 32:
        return (256, 32)
    if N <= 64:
        return (256, 64)
    if 128 < N <= 160:
        return (128, 160)
    return (128, 128)


def cb_lds_bytes(F):
    """csrc/cin_bwd.hip: two A and two B operand tiles, x0 and the dx0 row sums of the 128-row tile"""
    return 4 * (2 * CB_BK * CB_LDA + 2 * CB_BK * CB_LDB + 2 * F * CB_BM)


def fused_supported(M, Hk, Hp, F):
    """rn_cin_bwd_fused_supported (the sizes; rn_cin_bwd_fused_ok adds the 16-byte alignment of dX_k, W_k, x0t and the outputs)"""
    if M <= 0 or M % CB_BM or Hk < CB_BK or Hk % CB_BK or Hp not in (64, 128):
        return False
    if F < 4 or F % 4 or (F * Hp) % 128:
        return False
    if CB_BM * Hp > 2 * CB_BK * CB_LDA + 2 * CB_BK * CB_LDB:       # the join of dX_{k-1} aliases the operand buffers
        return False
    return cb_lds_bytes(F) <= 160 * 1024


def fused_layers(B, D, F, Hs, aligned=True):
    """per layer (0-based): does recnow_cin_bwd take the fused kernel"""
    ext = [F] + list(Hs)
    return tuple(bool(aligned) and fused_supported(B * D, ext[k + 1], ext[k], F) for k in range(len(Hs)))


def fwd_tags(Hs):
    return tuple(_TAG[pick_cfg(h)] for h in Hs)


def bwd_launches(fused):
    """hooked products of one backward call: dW_k, and the two data-gradient products where the fused kernel does not run"""
    return sum(1 if f else 3 for f in fused)


ROUTES = []
BOTH = ((1, 0), (0, 1))          # concat with the input kept; channel sum without it (k_rowsum overwrites on layer 1)
ALL4 = ((1, 1), (1, 0), (0, 1), (0, 0))


def row(name, why, fused, tags, B=8, D=16, F=4, Hs=(64, 32), modes=BOTH, census=(3, 3, 64)):
    ROUTES.append(dict(name=name, B=B, D=D, F=F, Hs=tuple(Hs), modes=tuple(modes), fused=tuple(bool(f) for f in fused), tags=tuple(tags),
                       census=tuple(census), why=why))


def spec(r):
    """the census spec of a row"""
    return dict(B=r['B'], D=r['D'], F=r['F'], Hs=r['Hs'])


row('ragged_general', 'M 15, F 7, H 5 / 3: every product on an edge kernel, nothing fused; all four output forms', (0, 0), (T256x32, T256x32),
    B=3, D=5, F=7, Hs=(5, 3), modes=ALL4)
row('fused64_shared', 'layer 1 with H_0 = F = 64: k_cin_bwd_fused<64>, one k-tile (H_1 32), two fields per column tile, dXp == dx0t', (1,),
    (T256x32,), F=64, Hs=(32,))
row('fused64_short', 'layer 2 on k_cin_bwd_fused<64> with NT = 2 k-tiles: both prefetch indices clamp; separate output buffers', (0, 1),
    (T256x64, T256x32), F=4, Hs=(64, 32))
row('fused128', 'layer 2 on k_cin_bwd_fused<128>: one field per column tile, two k-tiles (H_2 64), the wave columns split h', (0, 1),
    (T128, T256x64), F=4, Hs=(128, 64))
row('fused_lds_limit_f92', 'F 92: cb_lds_bytes = 160 000 <= 160 KiB, the largest F the fused kernel takes (46 column tiles)', (0, 1),
    (T256x64, T256x32), F=92, Hs=(64, 32))
row('lds_over_f96', 'F 96: cb_lds_bytes = 164 096 > 160 KiB: the same stack takes the two products', (0, 0), (T256x64, T256x32), F=96, Hs=(64, 32))
row('fallback_rows_b9', 'M 144 (M % 128 != 0): not fused', (0, 0), (T256x64, T256x32), B=9)
row('fallback_hk48', 'H_2 48 (H_k % 32 != 0): not fused', (0, 0), (T256x64, T256x64), Hs=(64, 48))
row('fallback_hp32', 'H_1 32 (H_{k-1} neither 64 nor 128): not fused', (0, 0), (T256x32, T256x32), Hs=(32, 32))
row('mixed_stack_12wg', 'M 1536: 12 workgroups; layer 1 on products (H_0 12), layer 2 on k_cin_bwd_fused<64> (four k-tiles), layer 3 on '
    'k_cin_bwd_fused<128>: both ping-pong buffers, seeds under the fused kernel and under the products', (0, 1, 1), (T256x64, T128, T256x32),
    B=96, F=12, Hs=(64, 128, 32))
row('family_256x32', 'H_2 16: 256 x 32 forward; H_k 16 < 32: not fused', (0, 0), (T256x64, T256x32), F=8, Hs=(64, 16))
row('family_256x64_l1', 'L 1, H_1 64: 256 x 64 forward, one layer (seed, dW and both products of layer 1 only)', (0,), (T256x64,), F=8, Hs=(64,))
row('family_128x128_l1', 'L 1, H_1 128: 128 x 128 forward', (0,), (T128,), F=8, Hs=(128,))
row('family_128x160', 'H_2 160: 128 x 160 forward; k_cin_bwd_fused<64> with five k-tiles per column tile', (0, 1), (T256x64, T160), F=8,
    Hs=(64, 160))
row('stride_loops', 'M 32 896 = 257 x 128: M F > 8192 x 256 (k_cin_in, k_cin_concat and their backward stride), k_rowsum beyond its 8192-block '
    'cap, 257 workgroups of k_cin_bwd_fused<64> with the shared buffer; dout on one row in rho', (1,), (T256x64,), B=4112, D=8, F=64, Hs=(64,),
    modes=((1, 1), (1, 0)))

# (census: every row keeps the first LADDER entry of tests/_cin_census.py; tests/test_cin_census_cpu.py checks that the ladder picks it)

MISALIGNED = dict(name='misaligned_w', B=8, D=16, F=4, Hs=(128, 64), modes=BOTH, fused=(False, False), tags=(T128, T256x64), census=(3, 3, 64),
                  why='every W_k one float into a larger buffer: sizes fit k_cin_bwd_fused<128>, the alignment does not: two products')

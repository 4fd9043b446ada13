"""The route table of the DCN-v2 layer (csrc/dcnmix.hip recnow_dcn_mix_fwd/bwd and recnow_dcn_mix_score_fwd/bwd): one row per distinct set of
kernels, with the call that reaches it.  Used by tests/test_mix_routes_gpu.py (on the GPU) and tests/test_mix_census_cpu.py (the census of every
row is exact).

How a call picks its kernels (csrc/dcnmix.hip, csrc/dcnmix_mid.hip, csrc/dcnmix_tile.hip):
  mix_exact              N S % 128 == 0, D % 128 == 0, B % 256 == 0, N <= 4, KP <= 512: the exact-128 formulation (LDT = KP); else the general
                         path (LDT = ldt_of: gate columns inside GEMM1, materialised x_{l+1}, unfused GEMM3 / dx products)
  rn_mix_mid_supported   S in {32, 64}, N <= 8, N (S / 32)^2 <= 16, LDT % 4 == 0, backward LDS <= 140 KB: k_mix_mid_fwd / _bwd (the _fast<S, N, slabs>
                         variants for (64, 2) and (32, 4) at LDT = N S + 16 and B % 32 == 0); else k_dcnmix_gate_fwd / _bwd + batched GEMMs
  rn_mix_mid_absorbs_slabs  (64, 2) or (32, 4), LDT = N S + 16, B % 32 == 0: a split-K GEMM1 / dT2g product leaves 2 or 4 slabs that the mid kernel sums
  mid_grid / mid_fwd_grid   at most 512 backward / 256 x (LDS per CU) forward workgroups: more 32-row tiles than that make workgroups walk several
  mix_tile_on            precision 0, RECNOW_TILE != 0, mix_tile_shape (exact, (64, 2), D in {256, 512, 1024}, B % 32 == 0, L <= 8), and
                         B <= 16 384 (or RECNOW_TILE=1): k_mix_tile_fwd; mix_tile_bwd_on (L <= 3, RECNOW_TILE_BWD != 0): k_mix_tile_bwd
  mix_tile_split_on      precision 1, mix_tile_shape, RECNOW_TILE_SPLIT=1: k_mix_tile_fwd_s3 (the backward stays on the product route)
  RECNOW_MIDF (per process)  N = 2, S = 64, LDT = 144, B % 128 == 0, B >= 65 536 rows or =2, precision 0: k_gemm<.., 25> (GEMM1 + sub-space forward)
  mix_xless (RECNOW_XLESS, per process)  exact, N <= 2, L > 1, below 512 row tiles (=2: at any batch, =0: off): x_{l+1} = x0 * O_l formed in
                         the operand loads of GEMM1 and dU
  mix_head_ok            exact, rn_mix_mid_supported, 2 D / 128 <= LDT: the score entry (fused Dense(1) head)
  the backward follows the forward's stamp of `saved` (which packs it left, xless, the route of the top piece)

Row fields: name, entry ('layer' | 'score'), B, D, S, N, L, prec (precision of the forward; bprec: of the backward when it differs), need_dx,
stream2 (the two-stream backward), call_env (per-call switches, set and restored around the row), proc_env (per-process switches: the row runs
in a child process with them), tags (recnow_prof tags of the route, of RN_TAG_MIX_MID_FWD/BWD, GEMM_SPLIT, GEMM_MIDF, MIX_TILE_FWD/BWD: exactly
these of the six appear), tile_route (recnow_dcn_mix_tile_route), corner (True: a row that exists for a dispatch corner only), why."""

MID_FWD, MID_BWD, SPLIT, MIDF, TILE_FWD, TILE_BWD = 6, 7, 8, 9, 10, 11       # csrc/prof.hpp RN_TAG_*
ROUTE_TAGS = frozenset((MID_FWD, MID_BWD, SPLIT, MIDF, TILE_FWD, TILE_BWD))

ROUTES = []


def row(name, why, entry='layer', B=512, D=384, S=64, N=2, L=2, prec=0, bprec=None, need_dx=1, stream2=False, call_env=None, proc_env=None,
        tags=(), tile_route=0, corner=False):
    ROUTES.append(dict(name=name, entry=entry, B=B, D=D, S=S, N=N, L=L, prec=prec, bprec=prec if bprec is None else bprec, need_dx=need_dx,
                       stream2=stream2, call_env=dict(call_env or {}), proc_env=dict(proc_env or {}), tags=frozenset(tags), tile_route=tile_route,
                       corner=corner, why=why))


def spec(r):
    """the census spec of a row"""
    return dict(B=r['B'], D=r['D'], S=r['S'], N=r['N'], L=r['L'], head=r['entry'] == 'score', need_dx=bool(r['need_dx']))


# ---- gate kernels + batched GEMMs ---------------------------------------------------------------------------------------------------------
row('gate_s8_n4_tails', 'S = 8: rn_mix_mid_supported refuses; B 300, D 200: not mix_exact (general path, edge GEMMs): k_dcnmix_gate_fwd/bwd',
    B=300, D=200, S=8, N=4, L=2)
row('gate_exact_n1_s128', 'N S = 128, KP = 144: mix_exact holds; S = 128: rn_mix_mid_supported refuses: gate kernels + batched GEMMs on the '
    'exact-128 route (L = 2, N = 1: xless)', B=256, D=128, S=128, N=1, L=2)
# ---- general path on the mid kernels (k_mix_dv_reduce behind the backward) --------------------------------------------------------------
row('mid_general_s32_n8', 'N = 8 > 4: not mix_exact; (32, 8) rn_mix_mid_supported: k_mix_mid_fwd<32>, k_mix_mid_bwd<32, 2>, k_mix_dv_reduce',
    B=512, D=256, S=32, N=8, L=1, tags=(MID_FWD, MID_BWD))
row('mid_general_s64_btail', 'B 300 (B % 256): not mix_exact, LDT 160 != 144: the general k_mix_mid_fwd<64>, k_mix_mid_bwd<64, 2>',
    B=300, D=256, S=64, N=2, L=2, tags=(MID_FWD, MID_BWD))
row('mid_general_s64_n1', 'N S = 64 (% 128 != 0): not mix_exact -- (64, 1) is a general-path shape -- k_mix_mid_fwd<64>, k_mix_mid_bwd<64, 1>',
    B=512, D=256, S=64, N=1, L=1, tags=(MID_FWD, MID_BWD))
# ---- exact product route on the mid kernels (D = 384 / 128: no row-block shape) --------------------------------------------------------------
row('mid_exact_64x2', 'exact, D 384 is no row-block shape, K = 384 < 512: no split: k_mix_mid_fwd_fast<64, 2, 0>, _bwd_fast<64, 2, false, 0>; '
    'L = 2, N = 2: xless', tags=(MID_FWD, MID_BWD))
row('mid_exact_32x4', 'exact (N S = 128, LDT 144): k_mix_mid_fwd_fast<32, 4, 0>, k_mix_mid_bwd_fast<32, 4, false, 0>', S=32, N=4,
    tags=(MID_FWD, MID_BWD))
row('mid_exact_64x4', 'exact (N S = 256, KP = LDT = 288): the general k_mix_mid_fwd<64>, k_mix_mid_bwd<64, 4> with deferred dV partials',
    B=256, D=128, S=64, N=4, L=1, tags=(MID_FWD, MID_BWD))
row('mid_slabs4_d1024', 'RECNOW_TILE=0, D 1024, 8 row tiles: GEMM1 and the dT2g product split into K / 256 = 4 slabs, absorbed: '
    'k_mix_mid_fwd_fast<64, 2, 4>, k_mix_mid_bwd_fast<64, 2, false, 4> (layer 0: the top layer\'s dT2g product writes dx = dy * O as a '
    'side output and is not split)', B=1024, D=1024, L=2, call_env={'RECNOW_TILE': '0'}, tags=(MID_FWD, MID_BWD))
row('mid_slabs2_32x4', 'D 512: K / 256 = 2 slabs absorbed by k_mix_mid_fwd_fast<32, 4, 2>, k_mix_mid_bwd_fast<32, 4, false, 2> (layer 0)',
    B=512, D=512, S=32, N=4, L=2, tags=(MID_FWD, MID_BWD))
row('mid_walk_25600', '800 tiles of 32 rows: more than mid_fwd_grid (3 x 256) and mid_grid (512) workgroups: workgroups walk several tiles '
    '(D 128: no row-block shape)', B=25600, D=128, L=1, tags=(MID_FWD, MID_BWD), corner=True)
# ---- midf and xless (per process) ------------------------------------------------------------------------------------------------------------
row('midf_l2', 'RECNOW_MIDF=2: N 2, S 64, LDT 144, B % 128 == 0 at any batch: GEMM1 with the sub-space forward in its epilogue (k_gemm<.., 25>), '
    'xless operand x0 * O_0 in it (RECNOW_XLESS=2)', proc_env={'RECNOW_MIDF': '2', 'RECNOW_XLESS': '2'}, tags=(MIDF, MID_BWD))
row('xless_off', 'RECNOW_XLESS=0: x_1 materialised between the layers (mid kernels)', proc_env={'RECNOW_XLESS': '0'}, tags=(MID_FWD, MID_BWD))
row('xless_off_tile', 'RECNOW_XLESS=0 on the row-block kernels: x_1 written by k_mix_tile_fwd', D=256, proc_env={'RECNOW_XLESS': '0'},
    tags=(TILE_FWD, TILE_BWD), tile_route=1)
# ---- row-block kernels ---------------------------------------------------------------------------------------------------------------------
row('tile_d256_l1', 'mix_tile_on: (64, 2), D 256, B <= 16 384: k_mix_tile_fwd + k_mix_tile_bwd', D=256, L=1, tags=(TILE_FWD, TILE_BWD), tile_route=1)
row('tile_d512_l2', 'row-block, D 512, L 2 (xless)', B=1024, D=512, L=2, tags=(TILE_FWD, TILE_BWD), tile_route=1)
row('tile_d1024_l3', 'row-block, D 1024, L 3 (both gradient ping-pong buffers)', B=512, D=1024, L=3, tags=(TILE_FWD, TILE_BWD), tile_route=1)
row('tile_l4_product_bwd', 'L = 4 > 3: mix_tile_bwd_on fails: row-block forward, product-route backward (packs made by the backward)',
    D=256, L=4, tags=(TILE_FWD, MID_BWD), tile_route=1)
row('tile_bwd_off', 'RECNOW_TILE_BWD=0: row-block forward, product-route backward', D=256, call_env={'RECNOW_TILE_BWD': '0'},
    tags=(TILE_FWD, MID_BWD), tile_route=1)
row('tile_walk_8448', '264 blocks of 32 rows on 256 workgroups: eight walk a second block', B=8448, D=256, L=2, tags=(TILE_FWD, TILE_BWD),
    tile_route=1, corner=True)
# ---- split precision -------------------------------------------------------------------------------------------------------------------------
row('split_l1', 'precision 1: no row-block route, RECNOW_TILE_SPLIT default off: split products (k_gemm_split: K = D 512 > 256, side product) '
    '+ mid kernels', D=512, L=1, prec=1,
    tags=(SPLIT, MID_FWD, MID_BWD))
row('split_l3', 'precision 1, L 3 (piece planes of every layer)', D=512, L=3, prec=1, tags=(SPLIT, MID_FWD, MID_BWD))
row('tile_split', 'RECNOW_TILE_SPLIT=1: k_mix_tile_fwd_s3, then the split product-route backward', D=256, prec=1,
    call_env={'RECNOW_TILE_SPLIT': '1'}, tags=(TILE_FWD, SPLIT, MID_BWD), tile_route=2)
row('flip_tile_fwd_split_bwd', 'forward at precision 0 (row-block, no product packs), backward at precision 1: the stamp makes the backward pack '
    'and take the split product route', D=256, prec=0, bprec=1, tags=(TILE_FWD, SPLIT, MID_BWD), tile_route=1)
row('flip_split_fwd_tile_bwd', 'forward at precision 1 (split GEMM1: K = D 512 > 256), backward at precision 0: row-block backward, tile packs '
    'made by it', D=512, prec=1, bprec=0, tags=(SPLIT, MID_FWD, TILE_BWD))
# ---- score entry (fused head) ----------------------------------------------------------------------------------------------------------------
row('score_mid_l1', 'score entry, product route, L 1: k_head_dx_top, rscale in k_mix_mid_bwd_fast, k_head_post', entry='score', L=1,
    tags=(MID_FWD, MID_BWD))
row('score_mid_l2', 'score entry, L 2, KP 144: dx written once (c2_mode 6)', entry='score', L=2, tags=(MID_FWD, MID_BWD))
row('score_mid_l3', 'score entry, L 3: dx written once (c2_mode 5)', entry='score', L=3, tags=(MID_FWD, MID_BWD))
row('score_mid_l4', 'score entry, L 4: the read-modify-write dx chain (c2_mode 4 on the top layer)', entry='score', B=256, D=128, L=4,
    tags=(MID_FWD, MID_BWD))
row('score_tile', 'score entry on the row-block kernels (head folded into k_mix_tile_fwd / _bwd)', entry='score', D=256,
    tags=(TILE_FWD, TILE_BWD), tile_route=1)
row('score_midf', 'score entry with RECNOW_MIDF=2: k_gemm<.., 25> + the head in GEMM3', entry='score', L=1,
    proc_env={'RECNOW_MIDF': '2', 'RECNOW_XLESS': '2'}, tags=(MIDF, MID_BWD))
# ---- other forms -----------------------------------------------------------------------------------------------------------------------------
row('no_dx_mid', 'need_dx = 0, dx = NULL: no O_l kept, no dx product', need_dx=0, tags=(MID_FWD, MID_BWD))
row('no_dx_score_tile', 'score entry, need_dx = 0 on the row-block kernels', entry='score', D=256, need_dx=0, tags=(TILE_FWD, TILE_BWD),
    tile_route=1)
row('stream2_mid', 'two-stream backward (stream2): weight-gradient products on the second stream', stream2=True, tags=(MID_FWD, MID_BWD))
row('stream2_tile', 'two-stream backward behind the row-block chain', D=256, L=3, stream2=True, tags=(TILE_FWD, TILE_BWD), tile_route=1)

# census data parameters of the rows (tests/_mix_census.py make: the first LADDER entry that keeps the row exact; checked on the CPU)
_CENSUS = {'mid_slabs4_d1024': (2, 2, 32), 'tile_d512_l2': (2, 2, 32), 'tile_d1024_l3': (1, 2, 16), 'tile_l4_product_bwd': (1, 1, 64), 'tile_walk_8448': (1, 2, 16),
           'split_l3': (1, 2, 16), 'score_mid_l3': (1, 2, 16), 'score_mid_l4': (1, 1, 64), 'stream2_tile': (1, 2, 16)}
for _r in ROUTES:
    _r['census'] = _CENSUS.get(_r['name'], (2, 2, 8))

PROC_ENVS = sorted({tuple(sorted(r['proc_env'].items())) for r in ROUTES if r['proc_env']})

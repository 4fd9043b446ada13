"""The route table of the exact-fp32 GEMM (csrc/gemm_dispatch.hpp rn_gemm_plan): one row per k_gemm instantiation of csrc/gemm_inst_lists.hpp and per
split-K reduce / XCD remap form, with the descriptor that reaches it.  Used by tests/test_gemm_plan_cpu.py (the planned kernel of every row, by
name, from recnow_gemm_route: no device), tests/test_gemm_routes_gpu.py (on the GPU, the same query for the very descriptor it launches) and
tests/test_exact_census_cpu.py (the census of every row is exact).

How a descriptor picks its kernel: rn_gemm_plan (csrc/gemm_dispatch.hpp, host-only) plans the whole route before anything is launched, and
rn_gemm_impl (csrc/gemm.hip) launches what the plan names; recnow_gemm_route returns the plan.  The plan's steps, in order:
  pick_cfg      N <= 32: 256 x 32;  N <= 64: 256 x 64;  128 < N <= 160: 128 x 160;  else 128 x 128
  wants_bm64    N = 128 with a side product (sp_r 1-2), batch 1, K >= 512, M % 64 == 0, at most 256 row tiles: 64 x 128 (lean64x, XF 9)
  pick_split    tiles < 512: ceil(512 / tiles) slices, capped at K / 256; else K >= 16384: K / 8192 slices (not with as_out / c_perm_s ...)
  bk16          K <= 256 on 128-row tiles (k-tiles of 16)
  gemm_interior M, N, K multiples of the tile and k-tile, 16-byte aligned operands and strides (else the EDGE kernel of the tile family)
  use_shortk    bk16 plain products (A [M][K], no operand mode, no bias, LINEAR, no c_trans, emul MUL or none, batch 1, no split, N tile 128)
                go to the persistent short-K kernel: a lean BK-16 row with A [M][K] and no operand mode carries a bias to stay on k_gemm
  XF            side product 1 (sp_r <= 2 at BK 32: the two-wide form 9; with staging 1 and A, B [k][row]: 41), rank-R update 2, as_out 5
  instantiated? the planned combination is looked up in the lists of csrc/gemm_inst_lists.hpp, the ones the launchers are expanded from: a lean
                combination without an instantiation runs the EDGE kernel of its family, one with XF is refused (RECNOW_EUNSUPPORTED)
  reduce        N % 4: variant 0; splitk >= 16, (total / 4) % 64 == 0 and < 96 blocks: variant 2; else 1
  xcd_remap     1: split, batch 1, one column tile, gridDim.z % 8 == 0, > 1 row tile;  2: > 1 column tile, gridDim.x % 8 == 0, no side product
  tag           the tile family of the planned kernel (precision 1: RN_TAG_GEMM_SPLIT only where a split kernel takes the product)
Row fields: (name, kernel, spec, extra, why).  spec: the census spec (tests/_exact_census.py); extra: off (A starts `off` floats into its
buffer, lda not a multiple of 4), tile (mt, nt): the census of (M / mt, K, N / nt) repeated mt x nt times (rows too large for a host census),
perm (c_perm_s), staging (recnow_set_gemm_staging), tag (tile family: RN_TAG_GEMM_*), reduce (variant; absent: one slice), remap (where the row
is about it).
Not in the table: XF 25 (the fused sub-space forward, reached by tests/test_midf_gpu.py through the layer oracle), the split-precision and the
short-K kernels (tests/test_split_routes_gpu.py).  Instantiated but never planned in exact mode: the BK-16 forms of XF 9, 41 and 25 (the plan
chooses those forms only when bk16 is false; tests/test_gemm_plan_cpu.py asserts it for every row)."""

T128, T160, T256x64, T256x32, T64 = 1, 2, 3, 4, 12          # csrc/prof.hpp RN_TAG_GEMM_*
TAG_SHORTK = 5
_WAVES = {(128, 128): (2, 2), (128, 160): (4, 1), (256, 64): (4, 1), (256, 32): (4, 1), (64, 128): (2, 2)}
_TAG = {(128, 128): T128, (128, 160): T160, (256, 64): T256x64, (256, 32): T256x32, (64, 128): T64}
RELU, TANH, SIGMOID = 1, 2, 3


def kname(bm, bn, bk, akc, bkc, edge, a2, b2, xf=0):
    wm, wn = _WAVES[(bm, bn)]
    b = lambda v: 'true' if v else 'false'      # noqa: E731
    return 'k_gemm<%d, %d, %d, %d, %d, %s, %s, %s, %d, %d, %d>' % (bm, bn, wm, wn, bk, b(akc), b(bkc), b(edge), a2, b2, xf)


ROUTES = []


def row(name, fam, bk, akc, bkc, edge, a2, b2, xf, why, extra=None, **spec):
    spec.setdefault('ta', 0 if akc else 1)
    spec.setdefault('tb', 1 if bkc else 0)
    if a2 > 0:
        spec['a_mode'] = a2
    if b2 > 0:
        spec['b_mode'] = b2
    e = dict(extra or {})
    e.setdefault('tag', _TAG[fam])
    ROUTES.append((name, kname(fam[0], fam[1], bk, akc, bkc, edge, a2, b2, xf), spec, e, why))


_COMBOS = [(True, False, 0, 0), (True, False, 3, 0), (True, True, 0, 0), (True, True, 1, 0), (True, True, 2, 0), (True, True, 3, 0),
           (False, False, 0, 0), (False, False, 1, 0), (False, False, 0, 2), (False, False, 0, 3)]


def _combo_spec(a2, b2, i):
    s = {}
    if a2 == 3:
        s['a_hq'] = 16
    if b2 == 3:
        s['b_hq'] = 16
    if a2 == 2:
        s['a_act'] = (TANH, SIGMOID, RELU)[i % 3]
    if b2 == 2:
        s['b_act'] = (SIGMOID, RELU, TANH)[i % 3]
    # spread the epilogue forms over the rows (bias / emul / accumulate / c_trans / act_cols)
    s.update([dict(bias=1), dict(e_mode=1), dict(accumulate=1), dict(c_trans=1), dict(bias=1, act_cols=100), dict(e_mode=2, e_act=TANH),
              dict(e_mode=2, e_act=SIGMOID), dict(bias=1, e_mode=1, accumulate=1), dict(), dict(e_mode=2, e_act=RELU)][i % 10])
    return s


# ---- lean 128 x 128 and 128 x 160 (gemm_inst_lean128.hip, gemm_inst_lean160.hip): 10 operand-kind combos x BK 16 / 32 ------------------------
for fam, N in (((128, 128), 128), ((128, 160), 160)):
    for i, (akc, bkc, a2, b2) in enumerate(_COMBOS):
        tn = 'lean%d' % fam[1]
        s = _combo_spec(a2, b2, i)
        row('%s_bk32_%d%d%d%d' % (tn, akc, bkc, a2, b2), fam, 32, akc, bkc, False, a2, b2, 0,
            'K = 384 > 256: k-tiles of 32; K < 512: one slice (K / 256 = 1)', M=256, N=N, K=384, **s)
        s = _combo_spec(a2, b2, i + 3)
        if akc and a2 == 0:
            s['bias'] = 1      # plain A [M][K] at BK 16 is the short-K kernel's unless there is a bias
        row('%s_bk16_%d%d%d%d' % (tn, akc, bkc, a2, b2), fam, 16, akc, bkc, False, a2, b2, 0,
            'K = 256 <= 256: k-tiles of 16%s' % (' (a bias keeps it off the short-K kernel)' if akc and a2 == 0 else ''), M=256, N=N, K=256, **s)

# ---- lean 256 x 64 (gemm_inst_lean64.hip) -------------------------------------------------------------------------------------------------
row('lean64_tf00', (256, 64), 32, True, False, False, 0, 0, 0, '32 < N = 64 <= 64: 256 x 64, A [M][K]', M=512, N=64, K=384, bias=1)
row('lean64_tt00', (256, 64), 32, True, True, False, 0, 0, 0, '256 x 64 with B [N][K]', M=512, N=64, K=384, e_mode=1, accumulate=1)
row('lean64_tf30_cin', (256, 64), 32, True, False, False, 3, 0, 0, "CIN's OUTER A operand on 256 x 64", M=512, N=64, K=384, a_hq=16, c_trans=1)

# ---- lean 128 x 128 with XF (gemm_inst_lean128x.hip) -------------------------------------------------------------------------------------
_XCOMBOS = [(True, False, 0, 0), (True, False, 1, 0), (True, True, 1, 0), (True, True, 0, 0), (False, False, 0, 0), (False, False, 1, 0)]
for i, (akc, bkc, a2, b2) in enumerate(_XCOMBOS):
    c = '%d%d%d%d' % (akc, bkc, a2, b2)
    row('x9_' + c, (128, 128), 32, akc, bkc, False, a2, b2, 9, 'side product sp_r 2, K = 384 < 512: wants_bm64 declines, BK 32: two-wide XF 9',
        M=256, N=128, K=384, sp_r=2, **_combo_spec(a2, b2, i))
    row('x1_bk16_' + c, (128, 128), 16, akc, bkc, False, a2, b2, 1, 'side product, K = 256: BK 16, no XF 9 at BK 16: XF 1',
        M=256, N=128, K=256, sp_r=2, **_combo_spec(a2, b2, i + 4))
    row('x1_bk32_sp%d_' % (3 + i % 2) + c, (128, 128), 32, akc, bkc, False, a2, b2, 1, 'sp_r > 2: the four-wide side product XF 1 at BK 32',
        M=256, N=128, K=384, sp_r=3 + i % 2, **_combo_spec(a2, b2, i + 7))
for akc, bkc in ((True, False), (True, True)):
    c = '%d%d00' % (akc, bkc)
    row('x2_bk32_' + c, (128, 128), 32, akc, bkc, False, 0, 0, 2, 'rank-R update eu_r 2, K = 384: one slice, BK 32', M=256, N=128, K=384, eu_r=2,
        bias=1, e_mode=1)
    row('x2_bk16_' + c, (128, 128), 16, akc, bkc, False, 0, 0, 2, 'rank-R update eu_r 3, K = 256: BK 16', M=256, N=128, K=256, eu_r=3,
        accumulate=1)
row('x2_longk_whole', (128, 128), 32, True, False, False, 0, 0, 2, 'rank-R update at K = 2048: 2 tiles would take 8 slices, but the slab reduce '
    'has no rank-R update: one slice', M=256, N=128, K=2048, eu_r=2, bias=1)
row('x5_bk32_1110', (128, 128), 32, True, True, False, 1, 0, 5, 'as_out: side product + A MUL + A-stream side output, BK 32', M=256, N=256, K=384,
    sp_r=2, as_out=1, bias=1)
row('x5_bk16_1110', (128, 128), 16, True, True, False, 1, 0, 5, 'as_out at K = 256: BK 16', M=256, N=128, K=256, sp_r=1, as_out=1)
row('x41_glds_0000', (128, 128), 32, False, False, False, 0, 0, 41, 'staging 1, A [K][M], B [K][N], sp_r 2, BK 32: LDS-DMA XF 41',
    {'staging': 1}, M=256, N=128, K=384, sp_r=2)

# ---- lean 64 x 128 (gemm_inst_lean64x.hip): wants_bm64 at its defaults ------------------------------------------------------------------
for i, (akc, bkc, a2, b2) in enumerate(_XCOMBOS):
    row('x9_bm64_%d%d%d%d' % (akc, bkc, a2, b2), (64, 128), 32, akc, bkc, False, a2, b2, 9,
        'N = 128, sp_r 2, K = 1024 >= 512, 8 row tiles of 128: 64 x 128; 16 tiles -> 4 slices, side columns in the slabs', {'reduce': 1},
        M=1024, N=128, K=1024, sp_r=2)

# ---- edge kernels (gemm_inst_edge.hip): 4 tile families x 4 layouts, M / N / K tails, A one float off its line (lda % 4 != 0) -----------------
_EDGE_SHAPES = {(256, 32): (300, 27), (256, 64): (300, 50), (128, 160): (200, 150), (128, 128): (200, 200)}
_EDGE_EXTRA = [dict(batch=2, bias=1, e_mode=1), dict(c_trans=1, accumulate=1), dict(bias=1, act_cols=13), dict(a_mode=3),
               dict(batch=3, accumulate=1, e_mode=2, e_act=SIGMOID), dict(a_mode=1, bias=1), dict(b_mode=2, b_act=TANH, act_cols=45),
               dict(a_mode=2, a_act=RELU, c_trans=1), dict(batch=2, b_mode=1, accumulate=1, bias=1), dict(e_mode=1, act_cols=1)]
_j = 0
for fam, (M, N) in _EDGE_SHAPES.items():
    for akc, bkc in ((True, False), (True, True), (False, False), (False, True)):
        s = dict(_EDGE_EXTRA[_j % len(_EDGE_EXTRA)])
        _j += 1
        if s.get('a_mode') == 3:      # an inner width that is not a multiple of 4 (the OUTER fast load needs hq % 4 == 0)
            cols = 77 if akc else M
            s['a_hq'] = next(h for h in (7, 5, 3) if cols % h == 0)
        a2, b2 = s.pop('a_mode', 0), s.pop('b_mode', 0)
        row('edge_%dx%d_%d%d' % (fam[0], fam[1], akc, bkc), fam, 32, akc, bkc, True, -1, -1, 0,
            'M %d, N %d, K 77 tails, A one float off (lda %% 4 = 1)' % (M, N), {'off': 1}, M=M, N=N, K=77, a_mode=a2, b_mode=b2, **s)

# ---- K split, slab reduce and XCD remaps -------------------------------------------------------------------------------------------------
row('split16_reduce_quad', (128, 128), 32, True, False, False, 0, 0, 0, '2 tiles, K 4096: 16 slices of 256; N % 4, 16 slices, 32 blocks: variant 2',
    {'reduce': 2}, M=256, N=128, K=4096, bias=1, e_mode=1, act_cols=100)
row('split256_k65536_quad', (128, 128), 32, False, False, False, 0, 0, 0, '2 tiles, K 65536: 256 slices of 256, variant 2',
    {'reduce': 2}, M=256, N=128, K=65536)
row('split8_batch_vec', (128, 128), 32, True, True, False, 0, 0, 0, 'batch 2: 4 tiles, K 2048: 8 slices < 16: variant 1',
    {'reduce': 1}, M=256, N=128, K=2048, batch=2, bias=1, e_mode=2, e_act=TANH, accumulate=1)
row('split8_ctrans_vec', (128, 128), 32, True, False, False, 0, 0, 0, '4 tiles, K 2048: 8 slices, variant 1, transposed store',
    {'reduce': 1}, M=256, N=256, K=2048, c_trans=1, accumulate=1, bias=1)
row('split32_edge_scalar', (128, 128), 32, True, False, True, -1, -1, 0, 'N 99 (N % 4 != 0): edge, 2 tiles, K 8192: 32 slices, variant 0',
    {'reduce': 0, 'off': 1}, M=256, N=99, K=8192, bias=1, e_mode=1)
row('split32_remap1', (128, 128), 32, False, False, False, 0, 0, 0, '8 row tiles x 1 column tile, 32 slices: gridDim.z % 8 == 0: xcd_remap 1',
    {'reduce': 1, 'remap': 1}, M=1024, N=128, K=8192, bias=1)
row('split32_cperm', (128, 128), 32, False, False, False, 0, 0, 0, 'dU-like x^T dA with c_perm_s 64: the permuted store of the reduce',
    {'reduce': 1, 'remap': 1, 'perm': 64}, M=1024, N=128, K=8192)
row('split_accuracy_k16384', (128, 128), 32, True, False, False, 0, 0, 0,
    '512 tiles fill the chip (no occupancy split), K 16384 >= 16384: 2 slices of 8192; 32 x 16 tiles: xcd_remap 2',
    {'reduce': 1, 'remap': 2, 'tile': (32, 16)}, M=4096, N=2048, K=16384)
row('remap2_nosplit', (128, 128), 32, True, True, False, 0, 0, 0, 'grid 8 x 2, K 384: one slice; gridDim.x % 8 == 0, no side product: xcd_remap 2',
    {'remap': 2}, M=1024, N=256, K=384, bias=1, e_mode=1)
row('kvalid_lean_bk16', (128, 128), 16, True, False, False, 0, 0, 0, 'K 144 with k_valid 130 (zero-padded last tile); bias: not short-K',
    M=256, N=128, K=144, k_valid=130, bias=1)
row('kvalid_edge', (128, 128), 32, True, False, True, -1, -1, 0, 'K 144 with k_valid 130, N 100: edge', M=256, N=100, K=144, k_valid=130,
    accumulate=1)


# ---- the descriptor of a row, as a function of the operands' base addresses -----------------------------------------------------------------
# tests/test_gemm_routes_gpu.py allocates one guard-banded device buffer per Geo and launches the descriptor; tests/test_gemm_plan_cpu.py hands the
# same function synthetic base addresses and asks recnow_gemm_route for the plan: both build the same descriptor.
PAD_ROWS = 256                    # a full tile of rows of guard band before and after every buffer
OUTER = 3


def _ceil4(n):
    return (n + 3) // 4 * 4


class Geo:
    """A (nb, rows, cols) matrix inside a guard-banded flat buffer of `words` floats: leading dimension ld, batch stride (rows + 1) * ld, PAD_ROWS rows
    before and after, the first element `off` floats into the buffer's lines.  rep: how often the stored data repeats along (rows, cols)."""

    def __init__(self, nb, rows, cols, ld, off=0, rep=(1, 1)):
        self.nb, self.rows, self.cols, self.ld, self.off, self.rep = nb, rows, cols, ld, off, rep
        self.sb, self.pre = (rows + 1) * ld, PAD_ROWS * ld + off
        self.words = self.pre + nb * self.sb + PAD_ROWS * ld + 64

    def ptr(self, base):
        return base + 4 * self.pre


def census_spec(spec, extra):
    """(the row's full spec, the spec of its host census: M / mt, N / nt under extra['tile'])"""
    from _exact_census import SPEC_DEFAULTS
    s = dict(SPEC_DEFAULTS)
    s.update(spec)
    mt, nt = extra.get('tile', (1, 1))
    return s, dict(s, M=s['M'] // mt, N=s['N'] // nt)


def stored_shapes(cs):
    """(batch, rows, cols) of the stored operand arrays A, A2, B, B2 of a census spec (tests/_exact_census.py _operands)"""
    out = {}
    for side in 'AB':
        if side == 'A':
            rows, cols = (cs['K'], cs['M']) if cs['ta'] else (cs['M'], cs['K'])
        else:
            rows, cols = (cs['N'], cs['K']) if cs['tb'] else (cs['K'], cs['N'])
        mode = cs['a_mode' if side == 'A' else 'b_mode']
        if mode == OUTER:
            hq = cs['a_hq' if side == 'A' else 'b_hq']
            out[side], out[side + '2'] = (1, rows, hq), (1, rows, cols // hq)
        else:
            out[side] = (cs['batch'], rows, cols)
            if mode:
                out[side + '2'] = out[side]
    return out


def geometry(s, extra, shapes):
    """name -> Geo of every buffer of the row's launch.  s: the full spec; shapes: stored_shapes of its census spec."""
    M, N, K, nb = s['M'], s['N'], s['K'], s['batch']
    mt, nt = extra.get('tile', (1, 1))
    off = extra.get('off', 0)
    g = {}
    for side in 'AB':
        _, rows, cols = shapes[side]
        rep = ((mt, 1) if side == 'A' else (1, nt)) if (mt, nt) != (1, 1) else (1, 1)
        o = off if side == 'A' else 0
        ld = _ceil4(cols * rep[1]) + 4 + (1 if o else 0)
        g[side] = Geo(shapes[side][0], rows * rep[0], cols * rep[1], ld, o, rep)
        mode = s['a_mode'] if side == 'A' else s['b_mode']
        if mode == OUTER:
            _, r2, c2 = shapes[side + '2']
            g[side + '2'] = Geo(1, r2, c2, _ceil4(c2) + 4)
        elif mode:
            g[side + '2'] = Geo(shapes[side + '2'][0], rows * rep[0], cols * rep[1], ld, o, rep)
    if extra.get('perm', 0):
        g['C'] = Geo(1, M * N // 128, 128, 128)
    elif s['c_trans']:
        g['C'] = Geo(nb, N, M, _ceil4(M) + 4)
    else:
        g['C'] = Geo(nb, M, N, _ceil4(N) + 4, rep=(mt, nt))
    if s['bias']:
        g['bias'] = Geo(nb, 1, N, _ceil4(N) + 4)
    if s['e_mode']:
        g['E'] = Geo(nb, M, N, _ceil4(N) + 4, rep=(mt, nt))
    if s['sp_r']:
        g['Bx'], g['Cx'] = Geo(1, K, s['sp_r'], s['sp_r'] + 4), Geo(1, M, s['sp_r'], s['sp_r'] + 4)
    if s['eu_r']:
        g['P'], g['Q'] = Geo(1, M, s['eu_r'], s['eu_r'] + 4), Geo(1, s['eu_r'], N, _ceil4(N) + 4)
    if s['as_out']:
        g['as_in'] = Geo(1, g['A'].rows, g['A'].cols, g['A'].ld)
        g['as_out'] = Geo(1, g['A'].rows, g['A'].cols, g['A'].ld)
    return g


def fill_desc(d, s, extra, act, geo, base):
    """Fills the recnow_gemm_desc `d` (rec_now_amd._lib.GemmDesc) of the row: geo from geometry(), base: name -> address of the buffer's first word."""
    p = {k: geo[k].ptr(base[k]) for k in geo}
    a, b, c = geo['A'], geo['B'], geo['C']
    d.A, d.lda, d.a_batch_stride, d.a_trans, d.a_mode, d.a_act = p['A'], a.ld, a.sb, s['ta'], s['a_mode'], s['a_act']
    d.B, d.ldb, d.b_batch_stride, d.b_trans, d.b_mode, d.b_act = p['B'], b.ld, b.sb, s['tb'], s['b_mode'], s['b_act']
    if s['a_mode']:
        d.A2 = p['A2']
    if s['b_mode']:
        d.B2 = p['B2']
    if s['a_mode'] == OUTER:
        d.a_hq, d.a_ld2 = s['a_hq'], geo['A2'].ld
    if s['b_mode'] == OUTER:
        d.b_hq, d.b_ld2 = s['b_hq'], geo['B2'].ld
    d.M, d.N, d.K, d.batch = s['M'], s['N'], s['K'], s['batch']
    d.C, d.ldc, d.c_batch_stride, d.c_trans, d.accumulate, d.c_perm_s = p['C'], c.ld, c.sb, s['c_trans'], s['accumulate'], extra.get('perm', 0)
    if s['bias']:
        d.bias, d.bias_batch_stride = p['bias'], geo['bias'].sb
    if s['e_mode']:
        d.emul, d.lde, d.e_batch_stride, d.e_mode, d.e_act = p['E'], geo['E'].ld, geo['E'].sb, s['e_mode'], s['e_act']
    d.act, d.act_cols, d.k_valid = act, s['act_cols'], s['k_valid']
    if s['sp_r']:
        d.sp_bx, d.sp_cx, d.sp_bx_ks, d.sp_bx_rs, d.sp_cx_ms, d.sp_cx_rs, d.sp_r = p['Bx'], p['Cx'], geo['Bx'].ld, 1, geo['Cx'].ld, 1, s['sp_r']
    if s['eu_r']:
        d.eu_p, d.eu_q, d.eu_pms, d.eu_qrs, d.eu_qns, d.eu_r = p['P'], p['Q'], geo['P'].ld, geo['Q'].ld, 1, s['eu_r']
    if s['as_out']:
        d.as_in, d.as_out = p['as_in'], p['as_out']
    return d


def planned_kernel(r):
    """the k_gemm instantiation a recnow_gemm_route_info names, spelled like the rows' `kernel` field (None: not a k_gemm launch)"""
    if r.family != 1:
        return None
    return kname(r.bm, r.bn, r.bk, r.a_kc, r.b_kc, r.edge, r.a2k, r.b2k, r.xf)


def check_route(name, kern, extra, r):
    """the planned route `r` (GemmRouteInfo) of a row's descriptor is the row's: kernel field by field, tag, reduce variant (no `reduce`: one slice) and
    the xcd_remap where the row states one"""
    assert planned_kernel(r) == kern, '%s: planned %s (family %d), the table says %s' % (name, planned_kernel(r), r.family, kern)
    assert r.tag == extra['tag'], '%s: planned tag %d, the table says %d' % (name, r.tag, extra['tag'])
    if 'reduce' in extra:
        assert r.splitk > 1 and r.reduce_variant == extra['reduce'], '%s: planned %d slices, reduce variant %d' % (name, r.splitk, r.reduce_variant)
    else:
        assert r.splitk == 1, '%s: planned %d slices, the table says one' % (name, r.splitk)
    if 'remap' in extra:
        assert r.xcd_remap == extra['remap'], '%s: planned xcd_remap %d, the table says %d' % (name, r.xcd_remap, extra['remap'])

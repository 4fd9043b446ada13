"""The route table of SENETLayer -- the fused kernels of csrc/senet_fused.hip and the four unfused entries of csrc/interact.hip -- one row per distinct
path with the call that reaches it, and a Python mirror of the two plan functions (sf_plan and senet_plan of the sources, queried through
recnow_senet_fused_route / _fused_grid and recnow_senet_route / _grid).  Used by tests/test_senet_routes_gpu.py (every row on the GPU against fp64 per
entry, and bit for bit on census data inside guard bands) and tests/test_senet_census_cpu.py (mirror == query; the table reaches every instantiation;
the census of every row is exact and has teeth).

fused (sf_ok: D % 4 == 0, Q = D / 4 a power of two, F Q <= 256, F <= 64, M <= 64)
  forward             D = 16, F % 8 == 0 and `out` on a 16-byte boundary: k_senet_fused_fwd8 (8 rows per step, at most 2048 workgroups: 16384 rows per pass;
                      F = M = 64 needs the LDS grant); else k_senet_fused_fwd (4 rows per step, at most 2048 workgroups: 8192 rows per pass).  P threads
                      share one hidden unit: P doubles from 1 while P < 8 and 2 P rows M <= 256, so P rows M <= 256 -- 8 up to M = 8, 4 up to 16, 2 up to
                      32 on 4 rows; 8 up to M = 4, 4 up to 8, 2 up to 16 on 8 rows
  backward            k_senet_fused_bwd<NACC>, NACC = 3 / 5 / 9 / 17 / 34 the first that holds ceil(nout / 256), nout = 2 F M + M + F; 4 rows per step, at
                      most min(2048, 256 x occupancy) workgroups
  rows                sf4_f1 (P = 8 > F = 1), sf4_q{1, 2, 4, 8, 16} (F Q < 256), sf4_q8_full / sf4_q16_full (F Q = 256: every thread a column), sf4_q4 is
                      D = 16 with F % 8 != 0, sf4_out_mis (D = 16, F = 8, out one float off: C ABI only), sf4_m{4, 5, 8, 9, 16, 17, 32, 33, 64} (P changes
                      at 8 | 9, 16 | 17 and 32 | 33), sf4_two_pass (B = 8197, F = 2, D = 4: workgroup 0 takes a whole second step, workgroup 1 a ragged one, the rest leave through
                      the clamped prefetch; two passes of the backward for any occupancy); sf8_m{2, 3, 4, 5, 8, 9, 16, 17, 33} on F = 8 / 16 / 64 (P changes at 4 | 5, 8 | 9, 16 | 17) (M = 33: 264
                      outputs, a second ragged round of the h loop), sf8_grant (F = M = 64), sf8_two_pass (B = 16395, F = 8); bwd_n{nout}: for every
                      instantiation the largest nout it serves and the smallest of the next that F, M <= 64 reach (bwd_edges() finds them), bwd_n768
                      (F = 14, M = 26), bwd_n8320 (F = M = 64: the last accumulator slot half used); sf_bias_{none, b1, b2, both} (one bias of two: C ABI
                      only; db1 / db2 are NULL where the bias is); sf_view_field / sf_view_dout (a field / the upstream gradient is a contiguous view one
                      float into a larger buffer: the layer hands the kernels aligned copies).  B cycles through 1, 3, 5 (4-row) and 1, 7, 9 (8-row); the
                      activation pair cycles so that every code stands in both positions in each of the three kernel families.
unfused (recnow_senet_squeeze / _scale_fwd / _scale_bwd_w / _scale_bwd_x, one choice for all four)
  uniform             uniform_d = D > 0 with D % 4 == 0, Q = D / 4 a power of two <= 64 and D F == total: k_senet_uniform<MODE>, ceil(B / 4) F Q items
                      on at most 16384 workgroups of 256
  tile                everything else: k_senet_tile<MODE> on R = min(32, floor(48 KiB / 4 (total + 1))) rows per workgroup, at most 4096 workgroups;
                      R < 1 (total > 12287): RECNOW_EUNSUPPORTED
  rows                uni_q{1 .. 64}: F = 65, F Q > 256 (what the layer sends there), B % 4 != 0, item counts that are no multiple of 256;
                      uni_two_pass (B = 1048578, F = 2, D = 32: 4194320 items, a second pass of 16; 67 M floats a tensor: census only, compared on the
                      device); tile_123, tile_5, tile_mixed, tile_6x5 (equal widths, no multiple of 4), tile_aligned_ud0 (equal aligned widths with
                      uniform_d = 0), tile_r32 / tile_r31 (total 383 / 384), tile_r12 (total 1000, B no multiple of 12), tile_r1 (total 12287, B = 3),
                      tile_two_pass (dims 1, 2, 3, B = 131109); uni_view_dout / tile_view_field (the layer with a misaligned upstream gradient / field)
Every loop has a one-pass row and a row with two passes whose last pass is ragged: k_senet_fused_fwd (sf4_* / sf4_two_pass), k_senet_fused_fwd8
(sf8_* / sf8_two_pass), k_senet_fused_bwd (bwd_* / sf4_two_pass, sf8_two_pass: NACC = 3; the loop is the same text in every instantiation),
k_senet_uniform (uni_q* / uni_two_pass) and k_senet_tile (tile_* / tile_two_pass).

Not in the table, on purpose: B = 0, a workspace one byte short, null pointers and total = 12288 launch nothing -- they are tests of their own in
tests/test_senet_routes_gpu.py, not rows; a second pass of k_senet_fused_bwd<5 .. 34> (the loop does not depend on NACC, and B = 8197 at F = M = 64
would be half a second of census arithmetic per run for no new code); a float4 kernel on a misaligned pointer (never run on purpose: the alignment
rows assert the pointers that reach the C call); callable activations (the unfused path with torch between the kernels: the excitation is then not a
kernel of this layer)."""
EUNSUPPORTED = -3
SF_FWD4, SF_FWD8, SF_BWD = 1, 2, 3
SENET_TILE, SENET_UNIFORM = 1, 2
SQUEEZE, SCALE, DW, DX = 0, 1, 2, 3
LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
ACT_NAMES = {LINEAR: 'linear', RELU: 'relu', TANH: 'tanh', SIGMOID: 'sigmoid'}
NACCS = (3, 5, 9, 17, 34)
OCC_ASSUMED = 8                              # the backward's grid follows the occupancy the runtime reports; without a device the mirror takes this one


# ---- mirrors --------------------------------------------------------------------------------------------------------------------------------------------
def sf_ok(F, D, M):
    if F < 1 or F > 64 or M < 1 or M > 64 or D < 4 or D % 4:
        return False
    q = D // 4
    return q & (q - 1) == 0 and F * q <= 256


def sf_split(rows, M):
    P = 1
    while P < 8 and 2 * P * rows * M <= 256:
        P *= 2
    return P


def sf8_ok(F, D, M):
    return D == 16 and 8 <= F <= 64 and F % 8 == 0 and 1 <= M <= 64


def nacc_of(F, M):
    need = (2 * F * M + M + F + 255) // 256
    return next((n for n in NACCS if need <= n), 34)


def fused_route(which, B, F, D, M, mis):
    if which not in (0, 1) or B < 0 or mis not in (0, 1):
        return -1
    if not sf_ok(F, D, M):
        return EUNSUPPORTED
    if B == 0:
        return 0
    if which == 1:
        return SF_BWD * 100000 + nacc_of(F, M)
    if sf8_ok(F, D, M) and not mis:
        lds = (2 * F * M + M + F + 8 * (2 * F + M) + 8 * 1040) * 4
        return SF_FWD8 * 100000 + sf_split(8, M) * 10 + int(lds > 64 * 1024)
    return SF_FWD4 * 100000 + sf_split(4, M) * 10


def fused_grid(which, B, F, D, M, mis, occ=OCC_ASSUMED):
    code = fused_route(which, B, F, D, M, mis)
    if code <= 0:
        return code
    rows = 8 if code // 100000 == SF_FWD8 else 4
    g = min(-(-B // rows), 2048)
    return min(g, 256 * occ) if which == 1 else g


def uniform_ok(D, F, total):
    if D < 4 or D % 4 or D * F != total:
        return 0
    q = D // 4
    return D if q & (q - 1) == 0 and q <= 64 else 0


def tile_rows(total):
    return min(32, (48 * 1024) // ((total + 1) * 4))


def senet_route(mode, B, F, total, ud):
    if mode not in (0, 1, 2, 3) or F < 1 or B < 0 or total < 1 or ud < 0:
        return -1
    if B == 0:
        return 0
    D = uniform_ok(ud, F, total)
    if D:
        return SENET_UNIFORM * 100000 + D // 4
    R = tile_rows(total)
    return EUNSUPPORTED if R < 1 else SENET_TILE * 100000 + R


def senet_grid(mode, B, F, total, ud):
    code = senet_route(mode, B, F, total, ud)
    if code <= 0:
        return code
    if code // 100000 == SENET_UNIFORM:
        return min(-(-(-(-B // 4) * (total // 4)) // 256), 16384)
    return min(-(-B // (code % 100000)), 4096)


def bwd_edges():
    """per instantiation: (F, M) of the largest nout it serves and of the smallest nout of the next one, over 1 <= F, M <= 64"""
    nouts = {}
    for F in range(1, 65):
        for M in range(1, 65):
            nouts.setdefault(2 * F * M + M + F, (F, M))
    edges = []
    for n in NACCS[:-1]:
        lim = 256 * n
        edges.append((n, max(v for v in nouts if v <= lim), min(v for v in nouts if v > lim)))
    return [(n, lo, nouts[lo], hi, nouts[hi]) for n, lo, hi in edges]


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------------
def geometry(r, occ=OCC_ASSUMED, bwd_grid=None):
    """what the restatement and the census need to know about the kernels of row r.  fused: per direction family, rows per step, P, Q, grid,
    stride = rows of one pass, passes (bwd_grid: the queried grid of the backward, else the mirror's at `occ`); unfused: family, Q or R, grid, stride,
    passes."""
    B = r['B']
    if r['kind'] == 'fused':
        g = {}
        for d, which in (('f', 0), ('b', 1)):
            code = r['fwd'] if which == 0 else r['bwd']
            fam = code // 100000
            rows = 8 if fam == SF_FWD8 else 4
            grid = fused_grid(which, B, r['F'], r['D'], r['M'], int(bool(r['out_lead'])), occ)
            if which == 1 and bwd_grid is not None:
                grid = bwd_grid
            e = dict(family=fam, rows=rows, P=sf_split(rows, r['M']), Q=r['D'] // 4, grid=grid, stride=grid * rows)
            e['passes'] = -(-B // e['stride'])
            if which == 1:
                e['nacc'] = code % 100000
            g[d] = e
        return g
    code = r['code']
    fam = code // 100000
    grid = senet_grid(0, B, len(r['dims']), sum(r['dims']), r['ud'])
    e = dict(family=fam, grid=grid)
    if fam == SENET_UNIFORM:
        e['Q'] = code % 100000
        qt = sum(r['dims']) // 4
        items, per = -(-B // 4) * qt, grid * 256
        e.update(items=items, per=per, passes=-(-items // per), stride=-(-per // qt) * 4)
    else:
        e['R'] = code % 100000
        e.update(stride=grid * e['R'], passes=-(-B // (grid * e['R'])))
    return {'u': e}


def pinned_rows(r):
    """rows that always carry gradient: the first and the last row and the first row of every pass of every kernel of the row"""
    rows = {0, r['B'] - 1}
    for e in geometry(r).values():
        rows |= set(range(0, r['B'], e['stride']))
    return sorted(rows)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
ROUTES = []
_ACTS = [(a, (a + a2) % 4) for a2 in range(4) for a in range(4)]       # every code in both positions within any four consecutive pairs
_count = {'f4': 0, 'f8': 0}


def fused(name, why, B, F, D, M, **kw):
    assert name not in {r['name'] for r in ROUTES}, name
    r = dict(kind='fused', name=name, why=why, B=B, F=F, D=D, M=M, dims=[D] * F, b1=True, b2=True, out_lead=0, view=None, census_only=False)
    r.update(kw)
    fam = 'f8' if (sf8_ok(F, D, M) and not r['out_lead']) else 'f4'
    if 'acts' not in r:
        r['acts'] = _ACTS[_count[fam] % 16]
        _count[fam] += 1
    r['fwd'] = fused_route(0, B, F, D, M, int(bool(r['out_lead'])))
    r['bwd'] = fused_route(1, B, F, D, M, 0)
    r['layer'] = r['b1'] == r['b2'] and not r['out_lead']               # one bias of two and a misaligned out: the C ABI alone
    ROUTES.append(r)
    return r


def unfused(name, why, B, dims, ud=None, **kw):
    assert name not in {r['name'] for r in ROUTES}, name
    F, total = len(dims), sum(dims)
    if ud is None:
        ud = dims[0] if len(set(dims)) == 1 and dims[0] % 4 == 0 else 0
    r = dict(kind='unfused', name=name, why=why, B=B, F=F, dims=list(dims), ud=ud, M=max(1, F // 2), acts=(RELU, SIGMOID), b1=True, b2=True, view=None,
             census_only=False, out_lead=0)
    r.update(kw)
    r['code'] = senet_route(0, B, F, total, ud)
    # the layer reaches the row's kernel when it does not fuse the shape and promises uniform_d exactly where the row does
    same = len(set(dims)) == 1 and dims[0] % 4 == 0
    r['layer'] = not r['census_only'] and not (same and sf_ok(F, dims[0], r['M'])) and (r['ud'] == (dims[0] if same else 0) or r['view'] == 'field')
    ROUTES.append(r)
    return r


def _expect(r, *codes):
    """the codes written out by hand next to the row (the mirror filled them in: a wrong mirror and a wrong expectation would have to agree)"""
    have = (r['fwd'], r['bwd']) if r['kind'] == 'fused' else (r['code'],)
    assert have == codes, (r['name'], have, codes)


def f4(P):
    return SF_FWD4 * 100000 + P * 10


def f8(P, grant=0):
    return SF_FWD8 * 100000 + P * 10 + grant


def bw(n):
    return SF_BWD * 100000 + n


# 4-row fused forward -------------------------------------------------------------------------------------------------------------------------------------
_expect(fused('sf4_f1', 'one field: P = 8 > F, seven of eight lanes of a hidden unit add nothing', 1, 1, 4, 1), f4(8), bw(3))
for _i, (_Q, _F, _M) in enumerate(((1, 3, 2), (2, 5, 3), (4, 7, 6), (8, 3, 2), (16, 2, 3))):
    _expect(fused('sf4_q%d' % _Q, 'Q = D / 4 = %d, F Q = %d < 256: idle threads past the row%s' % (_Q, _F * _Q, '; D = 16 with F %% 8 != 0' if _Q == 4 else ''),
                  (1, 3, 5)[_i % 3], _F, 4 * _Q, _M), f4(sf_split(4, _M)), bw(3))
_expect(fused('sf4_q8_full', 'F Q = 256 exactly at Q = 8: every thread a column', 5, 32, 32, 3), f4(8), bw(3))
_expect(fused('sf4_q16_full', 'F Q = 256 exactly at Q = 16', 3, 16, 64, 5), f4(8), bw(3))
_expect(fused('sf4_out_mis', 'D = 16, F = 8 with out one float off a 16-byte boundary: the 4-row kernel, whose float4 stores of out are then misaligned '
              'by 4 bytes -- dword-aligned vector stores, which gfx950 global memory takes (C ABI only)', 5, 8, 16, 3, out_lead=1), f4(8), bw(3))
for _i, (_M, _P) in enumerate(((4, 8), (5, 8), (8, 8), (9, 4), (16, 4), (17, 2), (32, 2), (33, 1), (64, 1))):
    _expect(fused('sf4_m%d' % _M, 'M = %d: P = %d in the 4-row kernels' % (_M, _P), (1, 3, 5)[_i % 3], 5, 8, _M), f4(_P), bw(nacc_of(5, _M)))
_expect(fused('sf4_two_pass', '8197 rows on 2048 workgroups of 4: workgroup 0 takes a whole second step, workgroup 1 one row of one, the others leave '
              'through the clamped prefetch; the backward makes at least two passes for any occupancy', 8197, 2, 4, 3), f4(8), bw(3))
# 8-row fused forward -------------------------------------------------------------------------------------------------------------------------------------
for _i, (_M, _P) in enumerate(((2, 8), (3, 8), (4, 8), (5, 4), (8, 4), (9, 2), (16, 2), (17, 1), (33, 1))):
    _F = (8, 16, 64)[_i % 3]
    _expect(fused('sf8_m%d' % _M, 'F = %d, M = %d: P = %d in k_senet_fused_fwd8%s' % (_F, _M, _P, '; 264 outputs: a second, ragged round of the h loop' if _M == 33 else ''),
                  (1, 7, 9)[_i % 3], _F, 16, _M), f8(_P), bw(nacc_of(_F, _M)))
_expect(fused('sf8_grant', 'F = M = 64 at D = 16: 72704 bytes of LDS, the grant', 9, 64, 16, 64), f8(1, 1), bw(34))
_expect(fused('sf8_two_pass', '16395 rows on 2048 workgroups of 8: workgroup 0 takes a whole second step, workgroup 1 three rows of one', 16395, 8, 16, 2),
        f8(8), bw(3))
# fused backward: both sides of every change of instantiation ----------------------------------------------------------------------------------------------
for _n, _lo, (_F1, _M1), _hi, (_F2, _M2) in bwd_edges():
    _next = NACCS[NACCS.index(_n) + 1]
    if _lo != 768:
        _expect(fused('bwd_n%d' % _lo, 'nout = %d: the largest k_senet_fused_bwd<%d> serves with F, M <= 64' % (_lo, _n), 5, _F1, 4, _M1), f4(sf_split(4, _M1)), bw(_n))
    _expect(fused('bwd_n%d' % _hi, 'nout = %d: the smallest of k_senet_fused_bwd<%d>' % (_hi, _next), 3, _F2, 4, _M2), f4(sf_split(4, _M2)), bw(_next))
_expect(fused('bwd_n768', 'nout = 768 = 3 x 256 exactly (F = 14, M = 26): every slot of k_senet_fused_bwd<3> used', 5, 14, 4, 26), f4(2), bw(3))
_expect(fused('bwd_n8320', 'F = M = 64: nout = 8320 = 32.5 x 256, the last used slot of k_senet_fused_bwd<34> half used, slot 33 never', 6, 64, 4, 64), f4(1), bw(34))
# biases (db1 / db2 are NULL where the bias is) ------------------------------------------------------------------------------------------------------------
for _nm, _b1, _b2 in (('none', False, False), ('b1', True, False), ('b2', False, True), ('both', True, True)):
    _expect(fused('sf_bias_%s' % _nm, 'b1 %s, b2 %s%s' % ('given' if _b1 else 'NULL', 'given' if _b2 else 'NULL', '' if _b1 == _b2 else ' (C ABI only)'), 5, 6, 8, 5,
                  b1=_b1, b2=_b2), f4(8), bw(3))
    _expect(fused('sf8_bias_%s' % _nm, 'the same on the 8-row kernel', 7, 8, 16, 5, b1=_b1, b2=_b2), f8(4), bw(3))
# alignment: the layer hands the float4 kernels aligned copies ---------------------------------------------------------------------------------------------
_expect(fused('sf_view_field', 'field 1 is a contiguous view one float into a larger buffer', 5, 3, 8, 2, view='field'), f4(8), bw(3))
_expect(fused('sf_view_dout', 'the upstream gradient is a contiguous view one float into a larger buffer', 5, 3, 8, 2, view='dout'), f4(8), bw(3))
_expect(fused('sf8_view_field', 'the same on the 8-row kernel', 9, 8, 16, 3, view='field'), f8(8), bw(3))
_expect(fused('sf8_view_dout', 'the same on the 8-row kernel', 9, 8, 16, 3, view='dout'), f8(8), bw(3))
# k_senet_uniform ------------------------------------------------------------------------------------------------------------------------------------------
for _Q, _F, _B in ((1, 65, 7), (2, 65, 5), (4, 70, 9), (8, 40, 6), (16, 17, 3), (32, 9, 5), (64, 5, 3)):
    _expect(unfused('uni_q%d' % _Q, 'Q = %d, F = %d (F > 64 or F Q > 256: what the layer sends to k_senet_uniform), %d items: ok is false inside the shuffles, '
                    'B %% 4 != 0' % (_Q, _F, -(-_B // 4) * _F * _Q), _B, [4 * _Q] * _F), SENET_UNIFORM * 100000 + _Q)
_expect(unfused('uni_two_pass', '1048578 rows of F = 2, D = 32: 4194320 items on 16384 x 256 threads, a second pass of 16 (census only: 67 M floats a tensor)',
                1048578, [32, 32], census_only=True), SENET_UNIFORM * 100000 + 8)
_expect(unfused('uni_view_dout', 'the layer with an upstream gradient one float into a larger buffer: cloned before the float4 kernels read it', 5, [4] * 65,
                view='dout'), SENET_UNIFORM * 100000 + 1)
# k_senet_tile ---------------------------------------------------------------------------------------------------------------------------------------------
_expect(unfused('tile_123', 'widths 1, 2, 3', 7, [1, 2, 3]), SENET_TILE * 100000 + 32)
_expect(unfused('tile_5', 'one field of 5', 1, [5]), SENET_TILE * 100000 + 32)
_expect(unfused('tile_mixed', 'widths 4, 8, 4, 32, 1', 65, [4, 8, 4, 32, 1]), SENET_TILE * 100000 + 32)
_expect(unfused('tile_6x5', 'equal widths that are no multiple of 4', 9, [6] * 5), SENET_TILE * 100000 + 32)
_expect(unfused('tile_aligned_ud0', 'equal aligned widths without the promise (uniform_d = 0): the tile kernels (C ABI; the layer: tile_view_field)', 5, [8] * 3, ud=0),
        SENET_TILE * 100000 + 32)
_expect(unfused('tile_view_field', 'the layer with field 1 one float into a larger buffer: no promise, the tile kernels on the misaligned field', 5, [4] * 65,
                ud=0, view='field'), SENET_TILE * 100000 + 32)
_expect(unfused('tile_r32', 'total = 383: the last total with R = 32', 33, [8] * 47 + [7]), SENET_TILE * 100000 + 32)
_expect(unfused('tile_r31', 'total = 384: R = 31, B no multiple of it', 33, [8] * 47 + [4, 4]), SENET_TILE * 100000 + 31)
_expect(unfused('tile_r12', 'total = 1000: R = 12, B no multiple of it', 29, [8] * 124 + [4, 4]), SENET_TILE * 100000 + 12)
_expect(unfused('tile_r1', 'total = 12287: one row per workgroup', 3, [8192, 2048, 1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1], layer_census=False),
        SENET_TILE * 100000 + 1)      # (a mean over 8192 columns times a gradient summed over 8192 columns needs 30 bits: the layer runs on random data only here)
_expect(unfused('tile_two_pass', '131109 rows on 4096 workgroups of 32: workgroup 0 takes 32 more, workgroup 1 five', 131109, [1, 2, 3]), SENET_TILE * 100000 + 32)

BY_NAME = {r['name']: r for r in ROUTES}
TOTAL_UNSUPPORTED = [8192, 4096]             # total = 12288: RECNOW_EUNSUPPORTED, nothing launched (a test of its own)

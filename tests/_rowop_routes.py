"""The route table of the three per-row ops -- FM (csrc/fm.hip), InnerPNN and attention_by_dot_product (csrc/interact.hip) -- one row per distinct
path, with the call that reaches it, and a Python mirror of the three route choices (fm_route, ipnn_route, attn_route of the sources, queried through
recnow_fm_route, recnow_inner_pnn_route, recnow_attention_dot_route).  Used by tests/test_rowop_routes_gpu.py (every row on the GPU against fp64 per
entry, and bit for bit on census data inside guard bands) and tests/test_rowop_census_cpu.py (mirror == query; the table reaches everything reachable;
the census of every row is exact and has teeth).

FM (nchunk = B D / 4 float4 chunks; a row is D / 4 = lanes_per_row consecutive chunks)
  vector shapes       D % 4 == 0 and D / 4 a power of two <= 64 (D in 4, 8, 16, 32, 64, 128, 256); every other D: k_fm_fwd_generic<SAVE_S> (one thread per
                      row, no loop) and k_fm_bwd_generic (grid-stride over B D elements, 2048 x 256 per pass)
  forward             nchunk >= 524288: k_fm_fwd_wide<SAVE_S, 4, 4> (1024 chunks per workgroup, at most 2048 workgroups: 2097152 chunks per pass);
                      else k_fm_fwd_vec4<SAVE_S> (256 chunks per workgroup, at most 2048 workgroups)
  backward            nchunk >= 524288 and nchunk % 1024 == 0: k_fm_bwd_wide<4, 4> (no tail code); else k_fm_bwd_vec4 (524288 chunks per pass)
  rows                generic: fm_generic_d5 / _d12 / _d260 / _d512 (one pass), fm_generic_two_pass (B D = 524500 > 524288: second pass of the backward);
                      vec4: fm_vec4_l1 .. fm_vec4_l64 (17 fields = two groups of 8 and one remainder field: the prefetch rotates once; B is no multiple of
                      the 256 / lanes rows of a workgroup: tail lanes), fm_f1; wide forward with a ragged tail + two-pass k_fm_bwd_vec4:
                      fm_wide_ragged_l1 .. _l64 (_l64 is D = 256, B = 8193, F = 5: one group of 4 and a remainder field); wide forward without a tail + wide
                      backward: fm_wide_exact_l1 .. _l64, fm_wide_bwd_f6 (remainder of 2), fm_wide_bwd_f9 (two groups: the prefetch rotates);
                      second pass of both wide kernels: fm_wide_two_pass (B = 32772: 256 chunks in pass 2, ragged) and fm_wide_bwd_two_pass (B = 32784:
                      2049 whole workgroups); SAVE_S = false (C ABI only, S = NULL, forward only): fm_nos_generic, fm_nos_vec4, fm_nos_wide
  never a second pass k_fm_fwd_vec4 and k_fm_fwd_generic: the launcher gives k_fm_fwd_vec4 nchunk < 524288 = 2048 workgroups x 256 only, so its grid of
                      ceil(nchunk / 256) <= 2048 workgroups covers every chunk in one pass; k_fm_fwd_generic has no loop (ceil(B / 256) workgroups)

InnerPNN (P = F (F - 1) / 2)
  Gram kernels        2 <= F <= 64 and D in {4, 8, 12, 16}: k_ipnn_fwd_gram<D> (two: F > 32 adds the g01 / g11 blocks; vec: P % 4 == 0 and out aligned ->
                      float4 stores) and k_ipnn_bwd_gram<D, NB, FULL> (NB = ceil(F / 16), FULL: F == 16 NB; vec: P % 4 == 0 and dout aligned); one wave per
                      row, 4 waves per workgroup, at most 16384 workgroups: 65536 rows per pass
  general kernels     every other shape with D <= 64: k_ipnn_fwd<DMAX> / k_ipnn_bwd<DMAX>, DMAX = 8 / 16 / 32 / 64 the next size above D; ipnn_cfg gives 4
                      waves per workgroup and halves while the waves' tiles exceed 64 KiB: (F DMAX + F (D + 1)) floats per wave forward, (F DMAX + P)
                      backward; nothing fits: RECNOW_EUNSUPPORTED (-3).  At most 4096 workgroups: 4096 x waves rows per pass
  rows                Gram: ipnn_gram_d{D}_f{F} for F = 16 NB (FULL, vec), 16 NB - 1 (P % 4 != 0: scalar) and 9 / 17 / 33 / 49 (not FULL, vec), and
                      ipnn_gram_d{D}_f{16 NB}_mis (dout and out one float off: FULL without vec), B in {1, 3, 5}; two passes: ipnn_gram_two_pass (B = 65540,
                      F = 3: scalar) and ipnn_gram_two_pass_vec (F = 9: the float4 requests of dout run ahead too).  General: ipnn_gen_d{5, 9, 17, 33} (4
                      waves), ipnn_gen_f70_d16 and ipnn_gen_f130_d4 (more than 64 fields: two and three column chunks; D % 4 == 0: float4 stores of dx),
                      ipnn_gen_f70_d16_mis_dx (the scalar dx stores k_ipnn_bwd falls back to inside the kernel when a dx buffer is misaligned), ipnn_gen_d{D}_f{F} (every F at
                      which a direction first runs on 2 / 1 waves -- all (DMAX, waves) pairs of both directions; where the backward tile no longer
                      fits bwd = -3 and the row runs forward only), ipnn_gen_two_pass (B = 16390, F = 2, D = 5)
  not in the table    F = 1: the forward is empty (code 0) and the backward is the general kernel writing zeros, the same instantiation as every other
                      general row of that D; B > 2^31 - 1 (the general kernels on a Gram shape) is beyond what a test can allocate

attention_by_dot_product
  float4 kernels      D % 4 == 0, CPL = D / 4 in {1, 2, 4, 8, 16} and every tensor aligned: k_attn_dot_v4<CPL, BWD>, 16 lanes per row, 16 rows per
                      workgroup, at most 8192 workgroups: 131072 rows per pass; ATTN_V4 = 4 pieces per lane and step: 64 pieces per row and step
  generic kernels     k_attn_dot_fwd / _bwd<GS>, GS = 16 / 32 / 64 for D <= 16 / <= 32 / <= 256; 256 / GS rows per workgroup: 131072 / 65536 / 32768 rows
                      per pass; GS = 64 keeps ATTN_NCH = 4 chunks of 64 columns
  rows                attn_v4_c{CPL}_nv{..}: L CPL = 64 and 64 + CPL pieces (and 63, 65 for CPL = 1) around the 64-piece step; attn_v4_two_pass,
                      attn_gs16_two_pass, attn_gs32_two_pass, attn_gs64_two_pass (the shapes of the issue: B just above one pass, ragged last row group);
                      attn_l0 (L = 0); attn_d{64, 65, 128, 129, 192, 193, 256} (v4 CPL 16, then 2, 3 and 4 live chunks of GS 64); attn_d3, attn_d17,
                      attn_d33, attn_d20 (CPL = 5 is no instantiation: GS 32); attn_mis_user (user_emb a view one float into a buffer: generic);
                      attn_*_dmat_only / _dsum_only (the other upstream gradient NULL), one of each per family

Every loop has a one-pass row and a row with at least two passes whose last pass is ragged: k_fm_fwd_wide (fm_wide_ragged_* / fm_wide_two_pass),
k_fm_bwd_wide (fm_wide_exact_* / fm_wide_bwd_two_pass: whole workgroups only, by its launch condition), k_fm_bwd_vec4 (fm_vec4_* / fm_wide_ragged_*),
k_fm_bwd_generic (fm_generic_d5 / fm_generic_two_pass), the Gram kernels (ipnn_gram_d* / ipnn_gram_two_pass*), the general InnerPNN kernels
(ipnn_gen_d5 / ipnn_gen_two_pass), k_attn_dot_v4 and the three GS (attn_v4_c* / attn_*_two_pass).

Row fields: op, name, B, F (attention: L), D, fwd / bwd (the expected route codes; bwd None: no backward is run), why, and per op: fm has_S; ipnn lead
(tensor -> floats past a 16-byte boundary: out, dout, dx); attn filter_neg, grads ('both', 'dmat', 'dsum') and lead (user, doc, mat, dmat, duser, ddoc);
view: the public entry point gets one input as a contiguous view one float into a larger buffer."""
EUNSUPPORTED = -3
FM_GENERIC, FM_VEC4, FM_WIDE = 1, 2, 3
IPNN_GENERAL, IPNN_GRAM_FWD, IPNN_GRAM_BWD = 1, 2, 3
ATTN_GENERIC, ATTN_V4 = 1, 2
ATTN_MIS = {'user': 1, 'doc': 2, 'mat': 4, 'dmat': 4, 'duser': 8, 'ddoc': 16}
FM_WIDE_MIN = 256 * 4 * 512                 # chunks: 512 workgroups of 4 per thread
FM_GRID_CAP = 2048
IPNN_GRAM_GRID, IPNN_GEN_GRID, ATTN_GRID = 16384, 4096, 8192
LDS = 64 * 1024


# ---- mirrors --------------------------------------------------------------------------------------------------------------------------------------------
def fm_vec_ok(D):
    lanes = D // 4
    return D % 4 == 0 and 1 <= lanes <= 64 and lanes & (lanes - 1) == 0


def fm_route(which, B, F, D, has_S):
    if which not in (0, 1) or F < 1 or B < 0 or D < 1 or has_S not in (0, 1) or (which == 1 and not has_S):
        return -1
    if B == 0:
        return 0
    save = 1 if (which == 0 and has_S) else 0
    if not fm_vec_ok(D):
        return FM_GENERIC * 100000 + save * 1000
    nchunk = B * D // 4
    wide = nchunk >= FM_WIDE_MIN and (which == 0 or nchunk % 1024 == 0)
    return (FM_WIDE if wide else FM_VEC4) * 100000 + save * 1000 + D // 4


def ipnn_cfg(F, D, bwd):
    """(DMAX, waves) of the general kernels, None where one row's tile does not fit"""
    dmax = 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else 64
    per_wave = (F * dmax + (F * (F - 1) // 2 if bwd else F * (D + 1))) * 4
    w = 4
    while w > 1 and per_wave * w > LDS:
        w >>= 1
    return None if per_wave * w > LDS else (dmax, w)


def ipnn_route(which, B, F, D, mask):
    if which not in (0, 1) or F < 1 or B < 0 or D < 1 or mask not in (0, 1):
        return -1
    if B == 0 or (which == 0 and F == 1):
        return 0
    if D > 64:
        return EUNSUPPORTED
    P = F * (F - 1) // 2
    if 2 <= F <= 64 and D in (4, 8, 12, 16) and B <= 0x7fffffff:
        vec = int(P % 4 == 0 and not mask)
        if which == 0:
            return IPNN_GRAM_FWD * 100000 + D * 100 + (F > 32) * 10 + vec
        nb = (F + 15) // 16
        return IPNN_GRAM_BWD * 100000 + D * 1000 + nb * 100 + (F == 16 * nb) * 10 + vec
    cfg = ipnn_cfg(F, D, which == 1)
    return EUNSUPPORTED if cfg is None else IPNN_GENERAL * 100000 + cfg[0] * 10 + cfg[1]


def attn_route(which, B, L, D, mask):
    if which not in (0, 1) or B < 0 or L < 0 or D < 1 or mask < 0 or mask > (31 if which else 7):
        return -1
    if D > 256:
        return EUNSUPPORTED
    if B == 0:
        return 0
    if D % 4 == 0 and not mask and D // 4 in (1, 2, 4, 8, 16):
        return ATTN_V4 * 100000 + D // 4
    return ATTN_GENERIC * 100000 + (16 if D <= 16 else 32 if D <= 32 else 64)


def masks(r):
    """(forward, backward) align_mask of a row"""
    ld = r.get('lead', {})
    if r['op'] == 'ipnn':
        return int(ld.get('out', 0) % 4 != 0), int(ld.get('dout', 0) % 4 != 0)
    if r['op'] == 'attn':
        bit = lambda *ks: sum(ATTN_MIS[k] for k in ks if ld.get(k, 0) % 4)      # noqa: E731
        return bit('user', 'doc', 'mat'), bit('user', 'doc', 'dmat', 'duser', 'ddoc')
    return 0, 0


def route(r, which, mask=None):
    """the mirror's answer for row r"""
    m = masks(r)[which] if mask is None else mask
    if r['op'] == 'fm':
        return fm_route(which, r['B'], r['F'], r['D'], 1 if which else int(r['has_S']))
    if r['op'] == 'ipnn':
        return ipnn_route(which, r['B'], r['F'], r['D'], m)
    return attn_route(which, r['B'], r['F'], r['D'], m)


def query(lib, r, which, mask=None):
    """the library's answer for row r"""
    m = masks(r)[which] if mask is None else mask
    if r['op'] == 'fm':
        return lib.recnow_fm_route(which, r['B'], r['F'], r['D'], 1 if which else int(r['has_S']))
    if r['op'] == 'ipnn':
        return lib.recnow_inner_pnn_route(which, r['B'], r['F'], r['D'], m)
    return lib.recnow_attention_dot_route(which, r['B'], r['F'], r['D'], m)


# ---- geometry: rows (or chunks) per pass of the grid-stride loops -------------------------------------------------------------------------------------
def _fm_grid(n):
    return max(1, min(-(-n // 256), FM_GRID_CAP))


def geometry(r):
    """what the restatement and the census need to know about the kernels row r runs on.  Per direction d in ('f', 'b'): family, and stride = rows of
    one pass of the kernel's loop (None: no loop); fm adds lanes, chunk strides and the field unroll, ipnn DMAX / NB / waves, attn CPL / GS."""
    op, B, F, D = r['op'], r['B'], r['F'], r['D']
    g = {}
    for d, code in (('f', r['fwd']), ('b', r['bwd'])):
        if code is None or code <= 0:
            g[d] = None
            continue
        fam = code // 100000
        e = dict(family=fam)
        if op == 'fm':
            lanes = code % 1000
            nchunk = B * D // 4
            e.update(lanes=lanes, fu=4 if fam == FM_WIDE else 8)
            if fam == FM_WIDE:
                e['cstride'] = _fm_grid(-(-nchunk // 4) if d == 'f' else nchunk // 4) * 1024
                e['block'] = 1024
            elif fam == FM_VEC4:
                e['cstride'] = _fm_grid(nchunk) * 256
                e['block'] = 256
            else:
                e['estride'] = None if d == 'f' else _fm_grid(B * D) * 256        # elements per pass of k_fm_bwd_generic
            e['stride'] = -(-e['cstride'] // lanes) if fam != FM_GENERIC else (None if d == 'f' else -(-e['estride'] // D))
        elif op == 'ipnn':
            if fam == IPNN_GENERAL:
                e.update(dmax=code // 10 % 1000, waves=code % 10)
                e['stride'] = min(-(-B // e['waves']), IPNN_GEN_GRID) * e['waves']
            else:
                e['stride'] = min(-(-B // 4), IPNN_GRAM_GRID) * 4
                if fam == IPNN_GRAM_BWD:
                    e['nb'] = code // 100 % 10
        else:
            if fam == ATTN_V4:
                e.update(cpl=code % 1000, rpw=4)
            else:
                e.update(gs=code % 1000, rpw=64 // (code % 1000))
            e['stride'] = max(1, min(-(-(-(-B // e['rpw'])) // 4), ATTN_GRID)) * 4 * e['rpw']
        g[d] = e
    return g


def pinned_rows(r):
    """rows that always carry gradient: the first and the last row (the last in-range row before a ragged tail), and the first row of every pass of
    the forward and of the backward kernel"""
    rows = {0, r['B'] - 1}
    for e in geometry(r).values():
        if e and e['stride']:
            rows |= set(range(0, r['B'], e['stride']))
    return sorted(rows)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
ROUTES = []


def row(op, name, why, B, F, D, **kw):
    assert name not in {r['name'] for r in ROUTES}, name
    r = dict(op=op, name=name, B=B, F=F, D=D, why=why, has_S=True, lead={}, filter_neg=False, grads='both', view=False)
    r.update(kw)
    r['fwd'] = route(r, 0)
    r['bwd'] = route(r, 1) if (op != 'fm' or r['has_S']) else None
    ROUTES.append(r)
    return r


def _expect(r, fwd, bwd):
    """the codes written out by hand next to the row (the mirror filled them in: a wrong mirror and a wrong expectation would have to agree)"""
    assert (r['fwd'], r['bwd']) == (fwd, bwd), (r['name'], r['fwd'], r['bwd'], fwd, bwd)


def fm_code(family, save, lanes):
    return family * 100000 + save * 1000 + lanes


# FM ------------------------------------------------------------------------------------------------------------------------------------------------------
for _D, _B, _F in ((5, 300, 3), (12, 70, 9), (260, 37, 9), (512, 9, 3)):
    _expect(row('fm', 'fm_generic_d%d' % _D, 'D = %d is no float4 shape: one thread per row; one pass of k_fm_bwd_generic' % _D, _B, _F, _D),
            fm_code(FM_GENERIC, 1, 0), fm_code(FM_GENERIC, 0, 0))
_expect(row('fm', 'fm_generic_two_pass', 'B D = 524500 elements on 2048 x 256 threads: the second pass of k_fm_bwd_generic, ragged', 104900, 2, 5),
        fm_code(FM_GENERIC, 1, 0), fm_code(FM_GENERIC, 0, 0))
for _l in (1, 2, 4, 8, 16, 32, 64):
    _expect(row('fm', 'fm_vec4_l%d' % _l, 'lanes_per_row = %d, %d rows on workgroups of %d rows: tail lanes; 17 fields = 8 + 8 + 1' % (
        _l, 2 * (256 // _l) + 1, 256 // _l), 2 * (256 // _l) + 1, 17, 4 * _l), fm_code(FM_VEC4, 1, _l), fm_code(FM_VEC4, 0, _l))
_expect(row('fm', 'fm_f1', 'one field: y = 0 exactly, dx = 0', 37, 1, 8), fm_code(FM_VEC4, 1, 2), fm_code(FM_VEC4, 0, 2))
for _l in (1, 2, 4, 8, 16, 32, 64):
    _B0 = FM_WIDE_MIN // _l
    _expect(row('fm', 'fm_wide_ragged_l%d' % _l, 'nchunk = 524288 + %d: k_fm_fwd_wide with a ragged tail, k_fm_bwd_vec4 with a second pass of one row' % _l,
                _B0 + 1, 5 if _l == 64 else 2, 4 * _l), fm_code(FM_WIDE, 1, _l), fm_code(FM_VEC4, 0, _l))
    _expect(row('fm', 'fm_wide_exact_l%d' % _l, 'nchunk = 524288 exactly: whole workgroups in k_fm_fwd_wide and k_fm_bwd_wide', _B0, 2, 4 * _l),
            fm_code(FM_WIDE, 1, _l), fm_code(FM_WIDE, 0, _l))
_expect(row('fm', 'fm_wide_bwd_f6', 'k_fm_bwd_wide with one group of 4 fields and a remainder of 2', 8192, 6, 256), fm_code(FM_WIDE, 1, 64), fm_code(FM_WIDE, 0, 64))
_expect(row('fm', 'fm_wide_bwd_f9', 'k_fm_bwd_wide with two groups of 4 (the prefetched group is rotated in) and a remainder of 1', 8192, 9, 256),
        fm_code(FM_WIDE, 1, 64), fm_code(FM_WIDE, 0, 64))
_expect(row('fm', 'fm_wide_two_pass', 'nchunk = 2097408 > 2048 x 1024: second pass of k_fm_fwd_wide with 256 chunks (4 rows); k_fm_bwd_vec4 makes 5 passes',
            32772, 2, 256), fm_code(FM_WIDE, 1, 64), fm_code(FM_VEC4, 0, 64))
_expect(row('fm', 'fm_wide_bwd_two_pass', 'nchunk = 2049 x 1024: workgroup 0 of k_fm_bwd_wide (and of k_fm_fwd_wide) makes a second pass', 32784, 2, 256),
        fm_code(FM_WIDE, 1, 64), fm_code(FM_WIDE, 0, 64))
_expect(row('fm', 'fm_nos_generic', 'S = NULL: k_fm_fwd_generic<false>', 300, 3, 5, has_S=False), fm_code(FM_GENERIC, 0, 0), None)
_expect(row('fm', 'fm_nos_vec4', 'S = NULL: k_fm_fwd_vec4<false>', 130, 9, 16, has_S=False), fm_code(FM_VEC4, 0, 4), None)
_expect(row('fm', 'fm_nos_wide', 'S = NULL: k_fm_fwd_wide<false, 4, 4> with a ragged tail', 8193, 5, 256, has_S=False), fm_code(FM_WIDE, 0, 64), None)
_expect(row('fm', 'fm_view', 'field 1 is a contiguous view one float into a larger buffer: FMLayer hands the kernels an aligned copy', 37, 3, 16, view=True),
        fm_code(FM_VEC4, 1, 4), fm_code(FM_VEC4, 0, 4))


# InnerPNN ------------------------------------------------------------------------------------------------------------------------------------------------
def gram_f(D, two, vec):
    return IPNN_GRAM_FWD * 100000 + D * 100 + two * 10 + vec


def gram_b(D, nb, full, vec):
    return IPNN_GRAM_BWD * 100000 + D * 1000 + nb * 100 + full * 10 + vec


def gen(dmax, waves):
    return IPNN_GENERAL * 100000 + dmax * 10 + waves


_n = 0
for _D in (4, 8, 12, 16):
    for _nb in (1, 2, 3, 4):
        _Bs = [(1, 3, 5)[(_n + i) % 3] for i in range(4)]
        _n += 1
        _Ff, _Fo, _Fv = 16 * _nb, 16 * _nb - 1, 16 * (_nb - 1) + (9 if _nb == 1 else 1)
        _expect(row('ipnn', 'ipnn_gram_d%d_f%d' % (_D, _Ff), 'F = 16 NB: FULL, P %% 4 == 0: float4 dout loads and result stores', _Bs[0], _Ff, _D),
                gram_f(_D, int(_Ff > 32), 1), gram_b(_D, _nb, 1, 1))
        _expect(row('ipnn', 'ipnn_gram_d%d_f%d_mis' % (_D, _Ff), 'FULL with out and dout one float off a 16-byte boundary: scalar stores and loads',
                    _Bs[1], _Ff, _D, lead={'out': 1, 'dout': 1}), gram_f(_D, int(_Ff > 32), 0), gram_b(_D, _nb, 1, 0))
        _expect(row('ipnn', 'ipnn_gram_d%d_f%d' % (_D, _Fo), 'F = 16 NB - 1: ragged last block, P %% 4 != 0: scalar', _Bs[2], _Fo, _D),
                gram_f(_D, int(_Fo > 32), 0), gram_b(_D, _nb, 0, 0))
        _expect(row('ipnn', 'ipnn_gram_d%d_f%d' % (_D, _Fv), 'one field (nine at NB = 1) in the last block, P %% 4 == 0: float4', _Bs[3], _Fv, _D),
                gram_f(_D, int(_Fv > 32), 1), gram_b(_D, _nb, 0, 1))
_expect(row('ipnn', 'ipnn_gram_two_pass', '65540 rows on 16384 workgroups of 4 waves: second pass of 4 rows; the next-row requests', 65540, 3, 4),
        gram_f(4, 0, 0), gram_b(4, 1, 0, 0))
_expect(row('ipnn', 'ipnn_gram_two_pass_vec', 'the same with P = 36: the float4 requests of dout run one pass ahead', 65540, 9, 4), gram_f(4, 0, 1), gram_b(4, 1, 0, 1))
_expect(row('ipnn', 'ipnn_view', 'field 1 is a contiguous view one float into a larger buffer: InnerPNNLayer hands the Gram kernels an aligned copy', 5, 9, 8,
            view=True), gram_f(8, 0, 1), gram_b(8, 1, 0, 1))
for _D, _dm in ((5, 8), (9, 16), (17, 32), (33, 64)):
    _expect(row('ipnn', 'ipnn_gen_d%d' % _D, 'D = %d: k_ipnn_fwd / _bwd<%d> on 4 waves' % (_D, _dm), 7, 11, _D), gen(_dm, 4), gen(_dm, 4))
# F at the first shape on which ipnn_cfg halves the waves, per direction: (F DMAX + P) x 4 bytes x waves <= 64 KiB backward, (F DMAX + F (D + 1)) x 4 forward;
# None: the backward tile of one wave is over 64 KiB, recnow_inner_pnn_bwd answers RECNOW_EUNSUPPORTED and the row runs forward only
for _D, _F, _wf, _wb in ((5, 84, 4, 2), (5, 121, 4, 1), (5, 293, 2, None), (5, 586, 1, None), (9, 77, 4, 2), (9, 114, 4, 1), (9, 158, 2, 1), (9, 316, 1, None),
                         (17, 65, 4, 2), (17, 82, 2, 2), (17, 101, 2, 1), (17, 164, 1, None), (33, 42, 2, 4), (33, 48, 2, 2), (33, 80, 2, 1), (33, 84, 1, 1)):
    _dm = 8 if _D <= 8 else 16 if _D <= 16 else 32 if _D <= 32 else 64
    _expect(row('ipnn', 'ipnn_gen_d%d_f%d' % (_D, _F), 'F = %d: the first F at which a direction of DMAX = %d loses waves (forward %d, backward %s)' % (
        _F, _dm, _wf, _wb or 'does not fit'), 3, _F, _D), gen(_dm, _wf), gen(_dm, _wb) if _wb else EUNSUPPORTED)
_expect(row('ipnn', 'ipnn_gen_f70_d16', 'F > 64 at a Gram width: general kernels, two 64-column chunks', 6, 70, 16), gen(16, 4), gen(16, 4))
_expect(row('ipnn', 'ipnn_gen_f70_d16_mis_dx', 'every dx buffer one float off a 16-byte boundary: k_ipnn_bwd<16> stores dx by scalars (its own test, no route)', 6, 70,
            16, lead={'dx': 1}), gen(16, 4), gen(16, 4))
_expect(row('ipnn', 'ipnn_gen_f130_d4', 'three 64-column chunks; the backward tile leaves one wave', 5, 130, 4), gen(8, 4), gen(8, 1))
_expect(row('ipnn', 'ipnn_gen_two_pass', '16390 rows on 4096 workgroups of 4 waves: second pass of 6 rows', 16390, 2, 5), gen(8, 4), gen(8, 4))

# attention_by_dot_product (F holds L) --------------------------------------------------------------------------------------------------------------------
_n = 0
for _c in (1, 2, 4, 8, 16):
    for _nv in ((63, 64, 65) if _c == 1 else (64, 64 + _c)):
        _n += 1
        _expect(row('attn', 'attn_v4_c%d_nv%d' % (_c, _nv), '%d float4 pieces per row around the 64-piece step of k_attn_dot_v4<%d>' % (_nv, _c), 5 + 2 * (_n % 3),
                    _nv // _c, 4 * _c, filter_neg=bool(_n % 2)), ATTN_V4 * 100000 + _c, ATTN_V4 * 100000 + _c)
_expect(row('attn', 'attn_v4_two_pass', '131075 rows on 8192 workgroups of 16 rows: second pass of 3 rows', 131075, 2, 4), 200001, 200001)
_expect(row('attn', 'attn_gs16_two_pass', '131075 rows, D = 5: second pass of k_attn_dot_fwd / _bwd<16>', 131075, 2, 5, filter_neg=True), 100016, 100016)
_expect(row('attn', 'attn_gs32_two_pass', '65540 rows, D = 20 (CPL = 5 is no instantiation): second pass of GS 32', 65540, 2, 20), 100032, 100032)
_expect(row('attn', 'attn_gs64_two_pass', '32770 rows, D = 65: second pass of GS 64, two live chunks', 32770, 2, 65, filter_neg=True), 100064, 100064)
_expect(row('attn', 'attn_l0', 'L = 0: zeros out, no user tensor is read', 5, 0, 8), 200002, 200002)
for _D, _fc in ((64, 200016), (65, 100064), (128, 100064), (129, 100064), (192, 100064), (193, 100064), (256, 100064)):
    _expect(row('attn', 'attn_d%d' % _D, 'D = %d: %s' % (_D, 'CPL 16' if _D == 64 else '%d live chunks of GS 64' % -(-_D // 64)), 3, 3, _D,
                filter_neg=_D in (65, 192)), _fc, _fc)
for _D, _fc in ((3, 100016), (17, 100032), (33, 100064), (20, 100032)):
    _expect(row('attn', 'attn_d%d' % _D, 'D = %d: GS %d with idle lanes' % (_D, _fc % 1000), 9, 5, _D, filter_neg=_D == 17), _fc, _fc)
_expect(row('attn', 'attn_mis_user', 'user_emb is a contiguous view one float into a larger buffer: the generic kernels in both directions', 9, 5, 8,
            lead={'user': 1}, view=True), 100016, 100016)
for _g in ('dmat', 'dsum'):
    _expect(row('attn', 'attn_v4_%s_only' % _g, 'the backward with only %s (the other upstream gradient NULL) on k_attn_dot_v4<4, true>' % _g, 9, 7, 16, grads=_g,
                filter_neg=_g == 'dsum'), 200004, 200004)
    _expect(row('attn', 'attn_gs_%s_only' % _g, 'the backward with only %s on k_attn_dot_bwd<32>' % _g, 9, 7, 18, grads=_g, filter_neg=_g == 'dmat'),
            100032, 100032)

BY_NAME = {r['name']: r for r in ROUTES}


def inputs(r):
    """input floats of a row (forward and backward)"""
    B, F, D = r['B'], r['F'], r['D']
    if r['op'] == 'fm':
        return B * F * D + B
    if r['op'] == 'ipnn':
        return B * F * D + B * F * (F - 1) // 2
    return B * F * D + 2 * B * D + B

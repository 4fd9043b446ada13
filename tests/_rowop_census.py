"""FM (csrc/fm.hip), InnerPNN and attention_by_dot_product (csrc/interact.hip) restated in numpy, for tests/test_rowop_routes_gpu.py and
tests/test_rowop_census_cpu.py.  Every output of the three ops depends on one batch row only.

  fm / ipnn / attn (.., dt=float64)
                    the closed form, with the cancellation-free magnitude of every sum next to it (scales=True).  The reference values of the GPU
                    test come from oracle/dense_ref under fp64 autograd; this form supplies the scales, and is held to the oracle by the CPU test.
                    Every sum is written `sum + 0.0`: the kernels add into a +0 accumulator, so a sum of -0 terms is +0.
  .. (.., dt=float32, geom=..)
                    the same in fp32 in the factorisation of the kernels of a table row (tests/_rowop_routes.py geometry()): per-lane partial sums
                    over the lane's float4, the butterfly over lanes_per_row / CPL / GS lanes, the sum over the positions of a lane group and the tree
                    over the groups (lanes c, c + CPL, ..), the k order of the MFMA steps.  What is inside one MFMA instruction (2 or 4 k slots) is
                    added left to right; compilers contract a * b + c: neither changes a census bit, and on random data both stay far inside the
                    half bound the CPU test holds the restatement to.  `mistake` plants one error (MISTAKES).
  make(r) / exact(c)
                    census data: integer inputs without a zero among them on which every sum any kernel forms keeps sum |terms| < 2^24, so fp32 in
                    ANY order gives the fp64 value to the bit.  Rows differ from row to row and InnerPNN's pair values from pair to pair, so a row or
                    a pair written to the wrong place changes bits.  Gradients are dense on pinned_rows() and hashed elsewhere.
  random_data(r)    N(0, 1) data for the comparison with fp64; with filter_neg every raw score is moved CLEAR x its magnitude away from 0."""
import zlib

import numpy as np

import _rowop_routes as T
from _dcn_census import EXACT, REL, same_bits        # noqa: F401  (the project's conventions: 2^24, 1e-5, bit equality with zero signs)

LADDER = [(3, 2), (2, 2), (2, 1), (1, 1)]              # (|x| in 1 .. xmax, |gradient| in 1 .. gmax): shrunk until every sum is exact
MISTAKES = {
    'fm': ('fm_tail_lane_stores', 'fm_remainder_dropped', 'fm_second_pass_skipped', 'fm_half_butterfly', 'fm_prefetch_not_rotated'),
    'ipnn': ('ipnn_pair_base_off_by_row', 'ipnn_g01_g11_dropped', 'ipnn_field_ge_F_stored', 'ipnn_UtX_missing', 'ipnn_prefetch_own_row'),
    'attn': ('attn_tail_pieces_counted', 'attn_filter_neg_passes_grad', 'attn_column_reduce_from_half', 'attn_dsum_left_out'),
}
KINK = 1e-4           # |raw score| >= KINK x sum_d |u_d doc_d| in the fp64 oracle (asserted by the callers): an fp32 dot product of D <= 256 terms is off by at
                      # most D x 2^-24 < 1.6e-5 of that magnitude, so fp32 sees the sign fp64 sees
CLEAR = 1e-2          # what random_data() clears


def _fold_halves(a, axis):
    """the xor butterfly `for (o = n / 2; o > 0; o >>= 1) v += shfl_xor(v, o)` as lane 0 sees it: lane i adds lane i + n / 2, then n / 4, .."""
    a = np.moveaxis(a, axis, -1)
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def _fold_pairs(a, axis):
    """the xor butterfly with growing offsets `for (o = 1; o < n; o <<= 1)`: neighbours first"""
    a = np.moveaxis(a, axis, -1)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def _seq(terms, axis, dt):
    """terms added one after the other into a +0 accumulator along `axis`"""
    terms = np.moveaxis(terms, axis, 0)
    acc = np.zeros(terms.shape[1:], dt)
    for t in terms:
        acc = acc + t
    return acc


# ---- FM -------------------------------------------------------------------------------------------------------------------------------------------------
def fm(x, g, dt=np.float64, geom=None, mistake=None, scales=False):
    """x (F, B, D), g (B,) or None (no backward).  Returns y (B,), S (B, D), dx (F, B, D); with scales s_y (B,), s_S and s_dx (B, D):
         y[b]        1/2 (sum_d (sum_f |x|)^2 + sum_{f,d} x^2)        S[b][d]   sum_f |x|        dx_f[b][d]   |g_b| sum_f |x_{f,b,d}|
    (dx_f = g (S - x_f): the one sum an entry of dx holds is S).  geom: geometry(row) of tests/_rowop_routes.py."""
    x = np.asarray(x, dt)
    F, B, D = x.shape
    res = {}
    gf = geom['f'] if geom else None
    gb = geom['b'] if geom else None
    nf = F
    if mistake == 'fm_remainder_dropped' and gf and gf['family'] != T.FM_GENERIC:
        nf = F - F % gf['fu']                                 # the `for (; f < F; ++f)` loop after the unrolled groups left out
    if gf is None:
        S = x.sum(0) + 0.0
        y = 0.5 * ((S * S - (x * x).sum(0)).sum(1) + 0.0)
    elif gf['family'] == T.FM_GENERIC:
        S, sq = np.zeros((B, D), dt), np.zeros((B, D), dt)
        for f in range(F):
            S, sq = S + x[f], sq + x[f] * x[f]
        y = dt(0.5) * _seq(S * S - sq, 1, dt)
    else:
        lanes = gf['lanes']
        xl = x.reshape(F, B, lanes, 4)
        s, sq = np.zeros((B, lanes, 4), dt), np.zeros((B, lanes, 4), dt)
        for f in range(nf):
            s, sq = s + xl[f], sq + xl[f] * xl[f]
        t = s * s - sq
        rl = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
        if mistake == 'fm_half_butterfly':
            assert lanes >= 2
            rl = rl[:, :lanes // 2]                           # the butterfly started at lanes_per_row / 4: lane 0 hears from half the row's lanes
        y = dt(0.5) * _fold_halves(rl, 1)
        S = s.reshape(B, D)
        nchunk = B * lanes
        if mistake == 'fm_second_pass_skipped' and nchunk > gf['cstride']:
            S = S.copy()
            S.reshape(-1)[gf['cstride'] * 4:] = 0
            y[gf['cstride'] // lanes:] = 0
        if mistake == 'fm_tail_lane_stores':
            # `ok` dropped from the stores, their index clamped as the load's: the lanes past the end, which all read chunk 0, store what they
            # computed at chunk 0 / row 0 -- S[chunk 0] again, and y[0] = half the butterfly over lanes_per_row copies of lane 0's partial.  (With the
            # index not clamped the stores land past the end: the guard bands of the GPU test see those.)
            assert nchunk % gf['block'] != 0
            y = y.copy()
            y[0] = dt(0.5) * _fold_halves(np.repeat(rl[:1, :1], rl.shape[1], 1), 1)[0]
    res.update(y=y, S=S)
    if g is not None:
        g = np.asarray(g, dt)
        src = np.arange(F)
        if mistake == 'fm_prefetch_not_rotated' and gb and gb['family'] != T.FM_GENERIC:
            fu = gb['fu']                                     # `v[u] = nv[u]` left out: every group of the unrolled loop subtracts the first group's fields
            assert F >= 2 * fu
            src[:F - F % fu] = src[:F - F % fu] % fu
        dx = g[None, :, None] * (S[None] - x[src])
        if mistake == 'fm_remainder_dropped' and gb and gb['family'] != T.FM_GENERIC:
            dx[F - F % gb['fu']:] = 0
        if mistake == 'fm_second_pass_skipped' and gb:
            per = gb['cstride'] * 4 if gb['family'] != T.FM_GENERIC else gb['estride']
            assert B * D > per or B * gf['lanes'] > gf['cstride']
            dx.reshape(F, -1)[:, per:] = 0
        res['dx'] = dx
    if scales:
        ax = np.abs(x)
        sa = ax.sum(0)
        res.update(s_y=0.5 * ((sa * sa).sum(1) + (x * x).sum((0, 2))), s_S=sa, s_dx=None if g is None else np.abs(g)[:, None] * sa)
    return res


# ---- InnerPNN -------------------------------------------------------------------------------------------------------------------------------------------
def pair_index(F):
    """(r, c) of pair p, r < c, r-major"""
    return np.triu_indices(F, 1)


def _T(r, F):
    """the kernels' pair-row base: pair (r, c) lives at T(r) + c"""
    return r * F - r * (r + 1) // 2 - r - 1


def _sym(dout, F, dt, upper_only=False):
    B = dout.shape[0]
    U = np.zeros((B, F, F), dt)
    ir, ic = pair_index(F)
    U[:, ir, ic] = dout
    if not upper_only:
        U[:, ic, ir] = dout
    return U


def ipnn(x, dout, dt=np.float64, geom=None, mistake=None, scales=False):
    """x (F, B, D), dout (B, P) or None.  Returns out (B, P), dx (F, B, D); with scales s_out (B, P) = sum_d |x_r x_c| and s_dx (F, B, D) =
    sum_{c != r} |dout_p| |x_c,d|."""
    x = np.asarray(x, dt)
    F, B, D = x.shape
    P = F * (F - 1) // 2
    ir, ic = pair_index(F)
    xb = np.ascontiguousarray(x.transpose(1, 0, 2))                              # (B, F, D)
    gf = geom['f'] if geom else None
    gb = geom['b'] if geom else None
    res = {}
    xf = xb
    if mistake == 'ipnn_prefetch_own_row' and gf:
        # the request for the next pass reads row bb instead of bb + nw: pass p computes on the rows of pass p - 1
        src = np.arange(B)
        assert B > gf['stride']
        src[gf['stride']:] -= gf['stride']
        xf = xb[src]
    if gf is None:
        G = np.einsum('brd,bcd->brc', xb, xb) + 0.0
    elif gf['family'] == T.IPNN_GRAM_FWD:
        hd = D // 2                                                              # v_mfma_f32_32x32x2: k slot h of step kk is element h D / 2 + kk
        G = np.zeros((B, F, F), dt)
        for kk in range(hd):
            G = (G + xf[:, :, None, kk] * xf[:, None, :, kk]) + xf[:, :, None, hd + kk] * xf[:, None, :, hd + kk]
    else:
        dm = gf['dmax']
        xp = np.zeros((B, F, dm), dt)
        xp[:, :, :D] = xf
        G = np.zeros((B, F, F), dt)
        for d in range(0, dm, 4):
            pr = [xp[:, :, None, d + i] * xp[:, None, :, d + i] for i in range(4)]
            G = G + (((pr[0] + pr[1]) + pr[2]) + pr[3])
    out = np.ascontiguousarray(G[:, ir, ic])
    if mistake == 'ipnn_pair_base_off_by_row':
        # base = T(r + 1) instead of T(r): every pair row lands F - r - 2 places further on, the tail of the last ones past P is lost
        bad = np.zeros((B, P), dt)
        for r in range(F - 1):
            idx = _T(r + 1, F) + np.arange(r + 1, F)
            ok = (idx >= 0) & (idx < P)
            bad[:, idx[ok]] = G[:, r, np.arange(r + 1, F)[ok]]
        out = bad
    if mistake == 'ipnn_g01_g11_dropped':
        assert F > 32                                                            # `if (two)` never taken: the columns 32 .. F - 1 are not computed
        out[:, ic >= 32] = 0
    if mistake == 'ipnn_field_ge_F_stored':
        # `j < F` dropped from `if (j > r && j < F) tile[base + jo] = g00[v]`: lanes j >= F store the product with a tile row no field was loaded into
        # (taken as 0 here) over the next pair rows, in the kernel's order: v = 0 .. 15, r = (v & 3) + 8 (v >> 2) + 4 h for both half waves h
        assert F <= 32
        tile = np.zeros((B, max(P, 64 * 20) + 64), dt)
        for v in range(16):
            for h in (0, 1):
                r = (v & 3) + 8 * (v >> 2) + 4 * h
                if r >= F - 1:
                    continue
                for j in range(r + 1, 32):
                    tile[:, _T(r, F) + j] = G[:, r, j] if j < F else 0
        out = np.ascontiguousarray(tile[:, :P])
    res['out'] = out
    if dout is not None:
        dout = np.asarray(dout, dt)
        xg, dg = xb, dout
        if mistake == 'ipnn_prefetch_own_row' and gb:
            src = np.arange(B)
            assert B > gb['stride']
            src[gb['stride']:] -= gb['stride']
            xg, dg = xb[src], dout[src]
        U = _sym(dg, F, dt)
        if gb is None:
            dx = np.einsum('bfg,bgd->bfd', U, xg) + 0.0
        elif gb['family'] == T.IPNN_GRAM_BWD:
            # v_mfma_f32_16x16x4: block I of 16 rows walks the k steps kk = 0 .. 4 NB - 1; the U X term where kk >= 4 I, then the U^T X term where
            # kk <= 4 I + 3, each over the 4 k slots 4 kk .. 4 kk + 3
            nb = gb['nb']
            Fp = 16 * nb
            Uu = np.zeros((B, Fp, Fp), dt)
            Uu[:, :F, :F] = _sym(dg, F, dt, upper_only=True)
            Ul = np.ascontiguousarray(Uu.transpose(0, 2, 1))
            if mistake == 'ipnn_UtX_missing':
                Ul = np.zeros_like(Ul)                                           # the `kk <= 4 * I + 3` MFMA left out
            xp = np.zeros((B, Fp, D), dt)
            xp[:, :F] = xg
            dxp = np.zeros((B, Fp, D), dt)
            for I in range(nb):
                rows = slice(16 * I, 16 * I + 16)
                acc = np.zeros((B, 16, D), dt)
                for kk in range(4 * nb):
                    for A, on in ((Uu, kk >= 4 * I), (Ul, kk <= 4 * I + 3)):
                        if on:
                            pr = [A[:, rows, 4 * kk + i, None] * xp[:, None, 4 * kk + i, :] for i in range(4)]
                            acc = acc + (((pr[0] + pr[1]) + pr[2]) + pr[3])
                dxp[:, rows] = acc
            dx = dxp[:, :F]
        else:
            if mistake == 'ipnn_UtX_missing':
                U = _sym(dg, F, dt, upper_only=True)
            dx = np.zeros((B, F, D), dt)
            for gcol in range(F):                                                # acc[d] += wgt * x_g[d], g = 0 .. F - 1
                dx = dx + U[:, :, gcol, None] * xg[:, None, gcol, :]
        res['dx'] = np.ascontiguousarray(dx.transpose(1, 0, 2))
    if scales:
        ab = np.abs(xb)
        res['s_out'] = np.einsum('brd,bcd->brc', ab, ab)[:, ir, ic]
        if dout is not None:
            res['s_dx'] = np.einsum('bfg,bgd->bfd', np.abs(_sym(dout, F, dt)), ab).transpose(1, 0, 2)
    return res


# ---- attention_by_dot_product ---------------------------------------------------------------------------------------------------------------------------
def attn(u, doc, dmat, dsum, filter_neg, dt=np.float64, geom=None, mistake=None, scales=False, backward=True):
    """u (B, L, D), doc (B, D), dmat (B, D) or None, dsum (B,) or None.  filter_neg: the score is max(s, 0) and its gradient passes where the raw
    score s > 0 -- none at s == 0 exactly, the kernels' convention (`if (!(sraw > 0.f)) ds = 0.f`; torch.clamp and tf.maximum pass it at the tie, which
    only integer census data ever hits).  Returns mat (B, D), ssum (B,), sraw (B, L), du (B, L, D), ddoc (B, D); with
    scales, S_l = sum_d |u_l,d doc_d| and A_l = sum_d |dmat_d u_l,d| + |dsum|:
         ssum  sum_l S_l      mat[d]  sum_l |u_l,d| S_l      du[l][d]  |dmat_d| S_l + A_l |doc_d|      ddoc[d]  sum_l A_l |u_l,d|"""
    u, doc = np.asarray(u, dt), np.asarray(doc, dt)
    B, L, D = u.shape
    gm = np.zeros((B, D), dt) if dmat is None else np.asarray(dmat, dt)
    gs = np.zeros(B, dt) if dsum is None or mistake == 'attn_dsum_left_out' else np.asarray(dsum, dt)
    gf = geom['f'] if geom else None
    gb = geom['b'] if geom else None

    def scores(ge, uu):
        """raw score and <dmat, u_l> per position, as the kernels of direction ge reduce them"""
        if ge is None:
            return (uu * doc[:, None]).sum(2) + 0.0, (uu * gm[:, None]).sum(2) + 0.0
        if ge['family'] == T.ATTN_V4:
            c = ge['cpl']
            u4, d4, g4 = uu.reshape(B, uu.shape[1], c, 4), doc.reshape(B, 1, c, 4), gm.reshape(B, 1, c, 4)
            lane = lambda pr: _fold_halves((pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3]), 2)       # noqa: E731
            return lane(u4 * d4), lane(u4 * g4)
        gsz = ge['gs']
        nch = 4 if gsz == 64 else 1
        pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (nch * gsz - D,), dt)], -1)                 # noqa: E731
        up, dp, gp = pad(uu).reshape(B, uu.shape[1], nch, gsz), pad(doc).reshape(B, 1, nch, gsz), pad(gm).reshape(B, 1, nch, gsz)
        return _fold_halves(_seq(up * dp, 2, dt), 2), _fold_halves(_seq(up * gp, 2, dt), 2)

    def over_positions(ge, terms):
        """sum over l of terms (B, L, ..) as direction ge accumulates it"""
        if ge is None:
            return terms.sum(1) + 0.0
        if ge['family'] != T.ATTN_V4:
            return _seq(terms, 1, dt)
        lpr = 16 // ge['cpl']                                  # position l sits on lane group l % lpr; the groups are added neighbours first
        n = terms.shape[1]
        pad = np.zeros((B, -n % lpr) + terms.shape[2:], dt)
        grp = np.concatenate([terms, pad], 1).reshape((B, -(-n // lpr), lpr) + terms.shape[2:])
        return _fold_pairs(_seq(grp, 1, dt), 1)

    def half_mix(ge, cols):
        """planted: the column reduce `for (o = CPL; o < 16; o <<= 1)` started at CPL / 2 -- lane c first adds the columns of lane c ^ (CPL / 2)"""
        c = ge['cpl']
        assert c >= 2
        v = cols.reshape(B, c, 4)
        return (v + v[:, np.arange(c) ^ (c // 2)]).reshape(B, D)

    uf = u
    if mistake == 'attn_tail_pieces_counted' and gf and gf['family'] == T.ATTN_V4:
        # `k < nv` dropped from the load, its index clamped into the row: the pieces between nv and the end of the 64-piece step read position 0
        # again and are counted into tot and the column sums
        nv = L * gf['cpl']
        extra = (-nv % 64) // gf['cpl']
        assert extra > 0
        uf = np.concatenate([u, np.repeat(u[:, :1], extra, 1)], 1)
    sraw, _ = scores(gf, uf)
    sc = np.maximum(sraw, 0) if filter_neg else sraw
    mat = over_positions(gf, uf * sc[..., None])
    ssum = over_positions(gf, sc)
    if mistake == 'attn_column_reduce_from_half' and gf and gf['family'] == T.ATTN_V4:
        mat = half_mix(gf, mat)
    res = dict(mat=mat, ssum=ssum, sraw=sraw[:, :L])
    if backward:
        sraw_b, q = scores(gb, u)
        scb = np.maximum(sraw_b, 0) if filter_neg else sraw_b
        ds = q + gs[:, None]
        if filter_neg and mistake != 'attn_filter_neg_passes_grad':
            ds = np.where(sraw_b > 0, ds, dt(0))
        res['du'] = gm[:, None, :] * scb[..., None] + ds[..., None] * doc[:, None, :]
        ddoc = over_positions(gb, ds[..., None] * u)
        if mistake == 'attn_column_reduce_from_half' and gb and gb['family'] == T.ATTN_V4:
            ddoc = half_mix(gb, ddoc)
        res['ddoc'] = ddoc
    if scales:
        au = np.abs(u)
        Sl = (au * np.abs(doc)[:, None]).sum(2)
        Al = (au * np.abs(gm)[:, None]).sum(2) + (0 if dsum is None else np.abs(np.asarray(dsum, dt))[:, None])
        res.update(s_ssum=Sl.sum(1), s_mat=(au * Sl[..., None]).sum(1), s_sraw=Sl,
                   s_du=np.abs(gm)[:, None, :] * Sl[..., None] + Al[..., None] * np.abs(doc)[:, None, :], s_ddoc=(Al[..., None] * au).sum(1))
    return res


# ---- one interface over the three ops -----------------------------------------------------------------------------------------------------------------
OUTPUTS = {'fm': ('y', 'S', 'dx'), 'ipnn': ('out', 'dx'), 'attn': ('mat', 'ssum', 'du', 'ddoc')}
FORWARD = {'fm': ('y', 'S'), 'ipnn': ('out',), 'attn': ('mat', 'ssum')}


def has_bwd(r):
    return r['bwd'] is not None and r['bwd'] > 0


def outputs(r):
    """what a call of row r writes (fm without S: y alone)"""
    if r['op'] == 'fm' and not r.get('has_S', True):
        return ('y',)
    return OUTPUTS[r['op']] if has_bwd(r) else FORWARD[r['op']]


def compute(r, d, dt=np.float64, restate=False, mistake=None, scales=False):
    """the op of row r on data d (a dict of its inputs); restate: in the factorisation of the row's kernels"""
    geom = T.geometry(r) if restate else None
    if r['op'] == 'fm':
        return fm(d['x'], d['g'] if has_bwd(r) else None, dt, geom, mistake, scales)
    if r['op'] == 'ipnn':
        return ipnn(d['x'], d['dout'] if has_bwd(r) else None, dt, geom, mistake, scales)
    return attn(d['u'], d['doc'], d.get('dmat'), d.get('dsum'), r['filter_neg'], dt, geom, mistake, scales)


def restate32(r, d, mistake=None):
    return compute(r, d, np.float32, True, mistake)


def margins(r, got, ref, sc, rel=REL):
    """worst |got - ref| / (rel x scale) per output that `got` holds, entry by entry against the entry's own scale; a scale of 0 demands an error of 0"""
    tiny = 1e-300
    m = {}
    for k in (k for k in outputs(r) if k in got):
        s = sc['s_' + k]
        if r['op'] == 'fm' and k == 'dx':
            s = s[None]
        m[k] = float((np.abs(np.asarray(got[k], np.float64) - ref[k]) / np.maximum(rel * s, tiny)).max()) if ref[k].size else 0.0
    return m


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def oracle(r, d):
    """the op of row r on data d through oracle/dense_ref in fp64, gradients by autograd"""
    import torch
    import dense_ref as R
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()            # noqa: E731
    if r['op'] in ('fm', 'ipnn'):
        xs = [t64(v).requires_grad_(True) for v in d['x']]
        if r['op'] == 'fm':
            y = R.fm_layer(xs)
            ref = dict(y=y.detach().numpy()[:, 0], S=torch.stack(xs).sum(0).detach().numpy())
            up = t64(d['g'])[:, None]
        else:
            y = R.inner_pnn_layer(xs)
            ref = dict(out=y.detach().numpy())
            up = t64(d['dout']) if has_bwd(r) else None
        if has_bwd(r):
            y.backward(up)
            ref['dx'] = np.stack([v.grad.numpy() for v in xs])
        return ref
    u, doc = t64(d['u']).requires_grad_(True), t64(d['doc']).requires_grad_(True)
    mat, ssum = R.attention_by_dot_product(u, doc, r['filter_neg'])
    outs, ups = [], []
    if 'dmat' in d:
        outs.append(mat)
        ups.append(t64(d['dmat']))
    if 'dsum' in d:
        outs.append(ssum)
        ups.append(t64(d['dsum'])[:, None])
    du, ddoc = torch.autograd.grad(outs, [u, doc], ups)
    return dict(mat=mat.detach().numpy(), ssum=ssum.detach().numpy()[:, 0], du=du.numpy(), ddoc=ddoc.numpy())


# ---- data -----------------------------------------------------------------------------------------------------------------------------------------------
def _nonzero(rng, hi, shape):
    return rng.integers(1, hi + 1, shape) * rng.choice([-1, 1], shape)


def _on(rng, r, rho=0.25):
    on = rng.random(r['B']) < rho
    on[T.pinned_rows(r)] = True
    return on


def _draw(r, xmax, gmax):
    rng = np.random.default_rng(zlib.crc32(('rowop census ' + r['name']).encode()))
    B, F, D = r['B'], r['F'], r['D']
    on = _on(rng, r)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)                      # noqa: E731
    if r['op'] == 'fm':
        return dict(x=f32(_nonzero(rng, xmax, (F, B, D))), g=f32(_nonzero(rng, gmax + 1, B) * on))
    if r['op'] == 'ipnn':
        return dict(x=f32(_nonzero(rng, xmax + 1, (F, B, D))), dout=f32(_nonzero(rng, gmax, (B, F * (F - 1) // 2)) * on[:, None]))
    d = dict(u=f32(_nonzero(rng, xmax, (B, F, D))), doc=f32(_nonzero(rng, xmax, (B, D))))
    if r['grads'] in ('both', 'dmat'):
        d['dmat'] = f32(_nonzero(rng, gmax, (B, D)) * on[:, None])
    if r['grads'] in ('both', 'dsum'):
        d['dsum'] = f32(_nonzero(rng, gmax, B) * on)
    return d


def sums_exact(r, d):
    """the largest sum |terms| over every sum the kernels form on this census (all of them must stay below 2^24)"""
    e = compute(r, d, scales=True)
    big = [float(np.max(v)) for k, v in e.items() if k.startswith('s_') and v is not None and np.size(v)]
    if r['op'] == 'fm':
        big.append(2 * float(e['s_y'].max()))                 # r = sum_d (s^2 - sq) before the halving; s^2 and sum x^2 are terms of it
    return max(big)


def make(r, params=None):
    """the census of route row r: the first LADDER entry on which every sum is exact (params: that entry, already known).  Returns (data, entry)."""
    for p in ([params] if params else LADDER):
        d = _draw(r, *p)
        if params or sums_exact(r, d) < EXACT:
            return d, p
    raise AssertionError('no census parameters keep %s exact' % r['name'])


def exact(r, d):
    return compute(r, d)


def random_data(r):
    """x, u, doc and the upstream gradients ~ N(0, 1).  Nothing here cancels beyond what the scales account for: every output entry is a sum whose
    scale is the sum of the magnitudes of its own terms, so centred data is as hard as any.  filter_neg: a position whose raw score s_l lies within
    CLEAR x S_l (S_l = sum_d |u_l,d doc_d|) of 0 in fp64 gets u_l moved along doc until |s_l| is 2 CLEAR x S_l -- a sign flip at the clamp is
    fp32's doing, not a kernel's; the callers assert KINK x S_l on the oracle."""
    rng = np.random.default_rng(zlib.crc32(('rowop random ' + r['name']).encode()))
    B, F, D = r['B'], r['F'], r['D']
    n32 = lambda *s: rng.normal(0, 1, s).astype(np.float32)                  # noqa: E731
    if r['op'] == 'fm':
        return dict(x=n32(F, B, D), g=n32(B))
    if r['op'] == 'ipnn':
        return dict(x=n32(F, B, D), dout=n32(B, F * (F - 1) // 2))
    d = dict(u=n32(B, F, D), doc=n32(B, D))
    if r['grads'] in ('both', 'dmat'):
        d['dmat'] = n32(B, D)
    if r['grads'] in ('both', 'dsum'):
        d['dsum'] = n32(B)
    if r['filter_neg'] and F:
        doc = d['doc'].astype(np.float64)
        for _ in range(20):
            u = d['u'].astype(np.float64)
            s = (u * doc[:, None]).sum(2)
            Sl = (np.abs(u) * np.abs(doc)[:, None]).sum(2)
            near = np.abs(s) < CLEAR * Sl
            if not near.any():
                break
            step = (np.where(s >= 0, 1.0, -1.0) * 2 * CLEAR * Sl - s) / (doc * doc).sum(1)[:, None]
            d['u'] = (u + (near * step)[..., None] * doc[:, None]).astype(np.float32)
    return d


def score_clearance(d):
    """smallest |s_l| / S_l of the raw scores in fp64 (inf without positions)"""
    u, doc = d['u'].astype(np.float64), d['doc'].astype(np.float64)
    if not u.size:
        return np.inf
    return float((np.abs((u * doc[:, None]).sum(2)) / (np.abs(u) * np.abs(doc)[:, None]).sum(2)).min())

"""Integer census of a whole CINLayer stack (csrc/cin.hip, csrc/cin_bwd.hip): forward, saved buffer and backward.

Every input is a small integer, chosen so that every intermediate of the forward and the backward pass -- every X_k, every seed of the output
gradient, every T = dX_k W_k, dX_k, dx0 and dW_k -- is an fp32 number and every sum a kernel forms -- over F H_{k-1}, over H_k, over f, over h,
over the kept channels, over the layers that add to dx0 and over the M = B D rows, in any order or split -- keeps the sum of the absolute values
of its terms below 2^24.  A correct kernel then returns the exact value to the bit; a kernel that drops a k-tile, loses a field parity, permutes
rows, seeds the wrong slice or accumulates onto a stale value does not.

Data (values from a per-element integer hash, tests/_exact_census.py `hash2`):
  emb      (B, F D), [b][f][d]: nonzero integers in +-[1, xmax]
  W_k      (H_k, F H_{k-1}): `k` entries +-1 per output channel at distinct hashed columns (f, h) -- not symmetric in (f, h)
  dout     +-1 on every row m = (b, d) when M <= 2048; above, on one hashed row in `rho` (always the first and the last row and at least one
           row of every 128-row block), 0 elsewhere: the M-deep sums of dW_k stay inside the window

`make(B, D, F, Hs, modes)` returns a Census whose parameters were shrunk along LADDER until the invariant holds in every mode of `modes`.
`expected(c, output_input, sum_channel)` is the exact result in fp64, evaluated through the sparse structure of W_k and on the rows with a
gradient.  `restate(c, output_input, sum_channel, order, mut)` is the layer in the kernels' factorisation -- per layer the fused form (T once,
then the reductions over f and over h) or the two products, as the route predicate says -- in fp64 or in fp32 in several summation orders, with an
optional planted mistake (MUTATIONS)."""
import numpy as np

from _exact_census import hash2, ints, exact32, WINDOW, frac_bits
from _cin_routes import fused_layers

BLOCK = 128                     # rows of a workgroup of k_cin_bwd_fused, and of a row tile of the dW product
DENSE_ROWS = 2048               # up to here every row carries a gradient
STALE = 3.0                     # what an accumulating k_rowsum finds in `out` (mutation rowsum_accumulates)


def _any_fused(s, hp=None):
    ext = [s['F']] + list(s['Hs'])
    return any(f and (hp is None or ext[k] == hp) for k, f in enumerate(fused_layers(s['B'], s['D'], s['F'], s['Hs'])))


# planted mistakes: name -> (what it models, applies(spec, output_input, sum_channel))
MUTATIONS = {
    'parity_lost': ('one field parity lost in the HP = 64 join of dX_{k-1}', lambda s, oi, sc: _any_fused(s, 64)),
    'drop_last_column_tile': ('the last column tile of T dropped', lambda s, oi, sc: _any_fused(s)),
    'drop_last_ktile': ('the last k-tile of the first column tile dropped', lambda s, oi, sc: _any_fused(s)),
    'ri_permuted': ('dx0 row sums land on permuted rows of their 32-row group (a wrong ri map)', lambda s, oi, sc: _any_fused(s)),
    'rowsums_not_added_shared': ('the dx0 row sums not added when dXp == dx0t', lambda s, oi, sc: fused_layers(s['B'], s['D'], s['F'], s['Hs'])[0]),
    'share_missing': ("X_{k-1}'s own share of the output gradient missing", lambda s, oi, sc: len(s['Hs']) > 1),
    'share_twice': ("X_{k-1}'s own share of the output gradient counted twice", lambda s, oi, sc: len(s['Hs']) > 1),
    'concat_offset_one_layer': ('the channel offset of a seed wrong by one layer (concat mode)', lambda s, oi, sc: not sc and len(s['Hs']) > 1),
    'input_share_missing': ('the input share of the output gradient missing (output_input)', lambda s, oi, sc: bool(oi)),
    'rowsum_accumulates': ('k_rowsum accumulates on the first kept layer, onto a stale value', lambda s, oi, sc: bool(sc)),
    'wt_swapped': ('Wt built with f and h swapped', lambda s, oi, sc: not all(fused_layers(s['B'], s['D'], s['F'], s['Hs']))),
    'drop_last_row': ('the last row dropped from dW', lambda s, oi, sc: True),
    'drop_last_block': ('the last 128-row block dropped from dW', lambda s, oi, sc: True),
    'in_bwd_transpose_swapped': ('the d / f transpose of k_cin_in_bwd swapped', lambda s, oi, sc: True),
}


def grad_rows(M, rho, salt=11):
    """rows m with a nonzero output gradient (see the module docstring)"""
    if M <= DENSE_ROWS:
        return np.ones(M, bool)
    on = (hash2((1, M, 1), salt)[0, :, 0] % np.uint64(rho)) == 0
    on[0] = on[-1] = True
    blk = np.arange(0, M, BLOCK)
    on[np.minimum(blk + (hash2((1, len(blk), 1), salt + 7)[0, :, 0] % np.uint64(BLOCK)).astype(np.int64), M - 1)] = True
    return on


def _weight(Hk, cols, k, salt):
    """(Hk, cols) float64: k entries +-1 per row at distinct hashed columns"""
    W = np.zeros((Hk, cols))
    pos = (hash2((1, k, Hk), salt) % np.uint64(cols)).astype(np.int64)[0]
    sign = np.where((hash2((1, k, Hk), salt + 1)[0] >> np.uint64(40)) & np.uint64(1), -1.0, 1.0)
    for c in range(Hk):
        for j in range(min(k, cols)):
            p = int(pos[j, c])
            while W[c, p] != 0:
                p = (p + 1) % cols
            W[c, p] = sign[j, c]
    return W


class Census:
    """spec: B, D, F, Hs.  params: (k, xmax, rho).  emb (B, F D), W[l] (H_l, F H_{l-1}): float32.  on: (M,) bool, the rows with a gradient.
    dout(oi, sc): float32 (B, D) or (B, ctot D)."""

    def ctot(self, oi):
        return (self.spec['F'] if oi else 0) + sum(self.spec['Hs'])

    def dout(self, oi, sc):
        B, D = self.spec['B'], self.spec['D']
        on = self.on.reshape(B, 1, D)
        C = 1 if sc else self.ctot(oi)
        g = ints((1, B, C * D), 13 + 2 * oi + sc, 1)[0].reshape(B, C, D) * on
        return g.reshape(B, C * D).astype(np.float32)


def make(B, D, F, Hs, modes=((1, 1), (1, 0), (0, 1), (0, 0)), params=None, verify=True):
    """A census of the stack.  params (k, xmax, rho) or None: the first LADDER entry for which the invariant holds in every mode."""
    spec = dict(B=B, D=D, F=F, Hs=tuple(Hs))
    M, ext = B * D, [F] + list(Hs)
    last = None
    for p in ([params] if params is not None else LADDER):
        k, xmax, rho = p
        c = Census()
        c.spec, c.params = spec, tuple(p)
        c.emb = ints((1, B, F * D), 3, xmax)[0].astype(np.float32)
        c.W = [_weight(ext[l + 1], F * ext[l], k, 100 * (l + 1)).astype(np.float32) for l in range(len(Hs))]
        c.on = grad_rows(M, rho)
        if not verify or B == 0:
            return c
        try:
            for oi, sc in modes:
                check_invariant(c, oi, sc)
        except AssertionError as e:
            last = e
            continue
        return c
    raise AssertionError('no census parameters keep %r exact: %s' % (spec, last))


# (entries per weight row, xmax, one row in rho carries a gradient beyond 2048 rows)
LADDER = ((3, 3, 64), (2, 3, 64), (2, 2, 64), (1, 2, 64), (1, 1, 64), (1, 1, 256))


# ---- arithmetic of a restatement -----------------------------------------------------------------------------------------------------------
class Exact:
    """fp64: exact for census data"""
    name, dtype = 'exact', np.float64

    def mm(self, A, B):
        return A @ B

    def rsum(self, T, axis):
        return T.sum(axis)


class Plain32(Exact):
    name, dtype = 'plain', np.float32

    def mm(self, A, B):
        return np.matmul(A.astype(np.float32), B.astype(np.float32))

    def rsum(self, T, axis):
        return T.astype(np.float32).sum(axis, dtype=np.float32)


class Reversed32(Plain32):
    name = 'reversed'

    def mm(self, A, B):
        return np.matmul(np.ascontiguousarray(A[:, ::-1], np.float32), np.ascontiguousarray(B[::-1], np.float32))

    def rsum(self, T, axis):
        return np.flip(T.astype(np.float32), axis).sum(axis, dtype=np.float32)


class Blocked32(Plain32):
    """products in k-tiles of 32 added last tile first, one fp32 add at a time; reductions as two parity partials (the HP = 64 join)"""
    name = 'blocked'

    def mm(self, A, B, blk=32):
        A, B = A.astype(np.float32), B.astype(np.float32)
        acc = None
        for k0 in reversed(range(0, A.shape[1], blk)):
            p = np.matmul(A[:, k0:k0 + blk], B[k0:k0 + blk])
            acc = p if acc is None else (acc + p).astype(np.float32)
        return acc

    def rsum(self, T, axis):
        T = np.moveaxis(T.astype(np.float32), axis, 0)
        odd = T[1::2].sum(0, dtype=np.float32)
        return (odd + T[0::2].sum(0, dtype=np.float32)).astype(np.float32) if T.shape[0] > 1 else T[0]


EXACT = Exact()
ORDERS = {o.name: o for o in (Plain32(), Reversed32(), Blocked32())}


def _ri_perm():
    """local row of a 32-row group -> the row a bit-reversed ri map sends its dx0 sum to (csrc/cin_bwd.hip: row = (ri & 3) + 8 (ri >> 2) + 4 h5)"""
    perm = np.zeros(32, np.int64)
    for h5 in range(2):
        for ri in range(16):
            wrong = ((ri & 1) << 3) | ((ri & 2) << 1) | ((ri & 4) >> 1) | ((ri & 8) >> 3)
            perm[(ri & 3) + 8 * (ri >> 2) + 4 * h5] = (wrong & 3) + 8 * (wrong >> 2) + 4 * h5
    return perm


def _outer(a, b):
    """Z[m][i * nb + j] = a[m][i] * b[m][j]"""
    return (a[:, :, None] * b[:, None, :]).reshape(a.shape[0], a.shape[1] * b.shape[1])


def restate(c, oi, sc, order=EXACT, mut=None, keep=False, fused=None, inp=None, tag=None):
    """The stack forward and backward in the kernels' factorisation.  order: the arithmetic (EXACT, ORDERS[..]).  fused: per layer, the fused
    form or the two products (default: what the sizes say).  inp: (emb, [W], dout) instead of the census data (dense, any values).
    tag: a name under which the forward of `inp` is kept with the census (the forward depends on neither the mode nor the mutation).
    Returns out, demb, dW0.., x0t, X1.. (and, with keep, T / dX of every layer under '_keep')."""
    s = c.spec
    B, D, F, Hs = s['B'], s['D'], s['F'], list(s['Hs'])
    M, L, ext = B * D, len(Hs), [F] + list(Hs)
    dt = order.dtype
    emb, Ws, dout = inp if inp is not None else (c.emb, c.W, c.dout(oi, sc))
    emb, Ws, dout = np.asarray(emb, dt), [np.asarray(w, dt) for w in Ws], np.asarray(dout, dt)
    fused = fused_layers(B, D, F, Hs) if fused is None else fused
    ctot = (F if oi else 0) + sum(Hs)
    res, kept = {}, {'T': [], 'dX': []}
    # ---- forward
    x0t = np.ascontiguousarray(emb.reshape(B, F, D).transpose(0, 2, 1)).reshape(M, F)
    key = (order.name, 'census' if inp is None else tag)
    cache = c.__dict__.setdefault('_fw', {})
    X = cache.get(key) if key[1] else None
    if X is None:
        X = []
        for l in range(L):
            Xp = x0t if l == 0 else X[l - 1]
            Wt_ = np.ascontiguousarray(Ws[l].T)
            X.append(np.concatenate([order.mm(_outer(x0t[m0:m0 + 2048], Xp[m0:m0 + 2048]), Wt_) for m0 in range(0, M, 2048)], 0).astype(dt))
        if key[1]:
            cache[key] = X
    layers = ([x0t] if oi else []) + X
    if sc:
        y = None
        for A in layers:
            r = order.rsum(A, 1)
            if y is None:
                y = (np.full(M, STALE, dt) + r).astype(dt) if mut == 'rowsum_accumulates' else r
            else:
                y = (y + r).astype(dt)
        res['out'] = y.reshape(B, D)
    else:
        res['out'] = np.ascontiguousarray(np.concatenate(layers, 1).reshape(B, D, ctot).transpose(0, 2, 1)).reshape(B, ctot * D)
    res['x0t'] = x0t
    for l in range(L):
        res['X%d' % (l + 1)] = X[l]
    # ---- backward, on the rows R that carry a gradient (every other row of every gradient is zero)
    if inp is None:
        on = c.on
    else:          # the rows with a gradient, and those with a non-finite input (0 * NaN: their gradients are not zero)
        with np.errstate(invalid='ignore'):
            on = (np.abs(dout.reshape(B, -1, D)).sum(1).reshape(M) != 0) | ~np.isfinite(x0t).all(1)
    R = np.flatnonzero(on)
    coffs = [0] + list(np.cumsum([F if oi else 0] + Hs))         # coffs[j]: channel offset of X_j in `out`, j >= 1 (x0t, when kept, sits at 0)
    g = dout.reshape(M) if sc else np.ascontiguousarray(dout.reshape(B, ctot, D).transpose(0, 2, 1)).reshape(M, ctot)

    def seed(j, shift=False):          # the gradient of `out` w.r.t. stored layer j, rows R
        H = ext[j]
        if sc:
            return np.repeat(g[R][:, None], H, 1)
        lo = coffs[j + 1] if shift else (coffs[j] if j > 0 else 0)
        return g[R][:, (lo + np.arange(H)) % ctot]
    dx0 = np.zeros((M, F), dt)
    if oi and mut != 'input_share_missing':
        dx0[R] = seed(0)
    x0R = x0t[R]
    dXk = seed(L)
    dwrows = np.ones(len(R), bool)
    if mut == 'drop_last_row':
        dwrows &= R != M - 1
    if mut == 'drop_last_block':
        dwrows &= R < BLOCK * ((M - 1) // BLOCK)
    perm = _ri_perm()
    for l in range(L - 1, -1, -1):
        Hk, Hp, W = ext[l + 1], ext[l], Ws[l]
        XpR = x0R if l == 0 else X[l - 1][R]
        res['dW%d' % l] = order.mm(np.ascontiguousarray(dXk[dwrows].T), _outer(x0R[dwrows], XpR[dwrows]))
        share = None
        if l > 0:
            share = seed(l, shift=(mut == 'concat_offset_one_layer'))
            share = {'share_missing': 0 * share, 'share_twice': (share + share).astype(dt)}.get(mut, share)
        if fused[l]:
            T = order.mm(dXk, W).astype(dt)
            if mut == 'drop_last_ktile':
                T[:, :128] = order.mm(dXk[:, :Hk - 32], W[:Hk - 32, :128]) if Hk > 32 else 0
            if mut == 'drop_last_column_tile':
                T[:, -128:] = 0
            T3 = T.reshape(len(R), F, Hp)
            t1 = (T3 * x0R[:, :, None]).astype(dt)
            if mut == 'parity_lost' and Hp == 64:
                t1 = t1[:, 0::2]
            a = order.rsum(t1, 1)                                                  # over f: dX_{k-1}
            b = order.rsum((T3 * XpR[:, None, :]).astype(dt), 2)                   # over h: dx0 row sums
            if keep:
                kept['T'].append(T)
            if l == 0:                       # dXp == dx0t: v = S + rs, then one update of the row
                v = a if mut == 'rowsums_not_added_shared' else (a + b).astype(dt)
                if mut == 'ri_permuted':
                    dx0[R] = (dx0[R] + a).astype(dt)
                    dx0[R - R % 32 + perm[R % 32]] += b
                else:
                    dx0[R] = (dx0[R] + v).astype(dt)
                dXp = None
            else:
                dXp = (share + a).astype(dt)
                if mut == 'ri_permuted':
                    dx0[R - R % 32 + perm[R % 32]] += b
                else:
                    dx0[R] = (dx0[R] + b).astype(dt)
        else:
            p1 = order.mm(_outer(dXk, x0R), W.reshape(Hk * F, Hp))                 # [(c, f)][h]
            Wt = W.reshape(Hk * Hp, F) if mut == 'wt_swapped' else np.ascontiguousarray(W.reshape(Hk, F, Hp).transpose(0, 2, 1)).reshape(Hk * Hp, F)
            p2 = order.mm(_outer(dXk, XpR), Wt)                                    # [(c, h)][f]
            if l == 0:
                dx0[R] = ((dx0[R] + p1).astype(dt) + p2).astype(dt)
                dXp = None
            else:
                dXp = (share + p1).astype(dt)
                dx0[R] = (dx0[R] + p2).astype(dt)
        if keep:
            kept['dX'].append(dXk)
        dXk = dXp
    if mut == 'in_bwd_transpose_swapped':
        res['demb'] = dx0.reshape(B, F * D).copy()
    else:
        res['demb'] = np.ascontiguousarray(dx0.reshape(B, D, F).transpose(0, 2, 1)).reshape(B, F * D)
    if keep:
        res['_keep'] = kept
    return res


def checked(c):
    """names of the outputs a GPU row compares"""
    return ['out', 'demb'] + ['dW%d' % l for l in range(len(c.spec['Hs']))]


def majorant(c, oi, sc, inp=None, fused=None):
    """The same computation on |emb|, |W|, |dout| (fp64): for every output and intermediate an upper bound of the sum of |terms| of every sum
    that leads to it, in any order or split."""
    emb, Ws, dout = inp if inp is not None else (c.emb, c.W, c.dout(oi, sc))
    a = (np.abs(np.asarray(emb, np.float64)), [np.abs(np.asarray(w, np.float64)) for w in Ws], np.abs(np.asarray(dout, np.float64)))
    return restate(c, oi, sc, inp=a, keep=True, fused=fused, tag='abs' if inp is None else None)


def check_invariant(c, oi, sc):
    """Integers everywhere and every majorant below 2^24: every intermediate and every partial sum of any order is an fp32 number."""
    for name, v in [('emb', c.emb), ('dout', c.dout(oi, sc))] + [('W', w) for w in c.W]:
        assert frac_bits(v.astype(np.float64)) == 0, '%s is not integral' % name
    maj = majorant(c, oi, sc)
    arrays = [(k, v) for k, v in maj.items() if k != '_keep'] + [('T', v) for v in maj['_keep']['T']] + [('dX', v) for v in maj['_keep']['dX']]
    for name, v in arrays:
        worst = float(v.max()) if v.size else 0.0
        assert worst < WINDOW, '%s: sum of |terms| %d >= 2^24' % (name, worst)
    for name, v in restate(c, oi, sc).items():
        assert exact32(v).all(), '%s is not an fp32 number' % name


# ---- the exact result, through the sparse structure --------------------------------------------------------------------------------------
def expected(c, oi, sc):
    """out, demb, dW0.., x0t, X1.. in fp64 (exact for census data): each W_k as its list of nonzero entries (c, f, h, v), the backward on the
    rows with a gradient; written from the layer's definition, not from the kernels' factorisation."""
    s = c.spec
    B, D, F, Hs = s['B'], s['D'], s['F'], list(s['Hs'])
    M, L, ext = B * D, len(Hs), [F] + list(Hs)
    x0t = c.emb.astype(np.float64).reshape(B, F, D).transpose(0, 2, 1).reshape(M, F)
    ent = []
    for l in range(L):
        ci, col = np.nonzero(c.W[l])
        ent.append((ci, col // ext[l], col % ext[l], c.W[l][ci, col].astype(np.float64)))
    X = [x0t]
    for l in range(L):
        ci, fi, hi, v = ent[l]
        Xk = np.zeros((ext[l + 1], M))
        np.add.at(Xk, ci, v[:, None] * x0t.T[fi] * X[l].T[hi])
        X.append(np.ascontiguousarray(Xk.T))
    layers = X if oi else X[1:]
    cat = np.concatenate(layers, 1)
    ctot = cat.shape[1]
    res = {'x0t': x0t}
    res['out'] = cat.sum(1).reshape(B, D) if sc else cat.reshape(B, D, ctot).transpose(0, 2, 1).reshape(B, ctot * D)
    for l in range(L):
        res['X%d' % (l + 1)] = X[l + 1]
    dout = c.dout(oi, sc).astype(np.float64)
    R = np.flatnonzero(c.on)
    gcat = (np.repeat(dout.reshape(M, 1), ctot, 1) if sc else dout.reshape(B, ctot, D).transpose(0, 2, 1).reshape(M, ctot))[R]
    offs = np.cumsum([0] + [a.shape[1] for a in layers])
    dX = [None] * (L + 1)                      # gradient w.r.t. stored layer j on rows R: its share of `out` ...
    for j in range(L + 1):
        i = j if oi else j - 1
        dX[j] = gcat[:, offs[i]:offs[i + 1]].copy() if i >= 0 else np.zeros((len(R), F))
    xR = x0t[R]
    for l in range(L - 1, -1, -1):             # ... plus what flows back through layer l + 1
        ci, fi, hi, v = ent[l]
        XpR = X[l][R]
        t = v[None, :] * dX[l + 1][:, ci]                       # (rows, entries)
        res['dW%d' % l] = dX[l + 1].T @ (xR[:, :, None] * XpR[:, None, :]).reshape(len(R), -1)
        np.add.at(dX[l].T, hi, (t * xR[:, fi]).T)
        np.add.at(dX[0].T, fi, (t * XpR[:, hi]).T)
    dx0 = np.zeros((M, F))
    dx0[R] = dX[0]
    res['demb'] = dx0.reshape(B, D, F).transpose(0, 2, 1).reshape(B, F * D)
    return res


# ---- the fused kernel's summation orders in fp32, for the per-product constant of the random-data bound ---------------------------------------
# Per-product constant of k_cin_bwd_fused on random data, |err|_i <= C_FUSED (sum of |terms|)_i.  Its orders differ from a GEMM's: an H_k-deep
# fma chain for T, then a chain over the fields of a parity (dX_{k-1}) or two-term partials and a tree over 32 lanes (dx0).  The host fp32
# emulation of these orders below, against fp64 (x ~ N(0, 0.5), W ~ U(-0.5, 0.5), 128 rows, at the (H_k, H_{k-1}, F) of every fused layer of
# tests/_cin_routes.py), gave at most C_FUSED_MEASURED (the worst at H_k 64, H_{k-1} 128, F 4; tests/test_cin_census_cpu.py test_fused_constant
# repeats the measurement).  C_FUSED is 2.4x that, the margin the GEMM constant C_ELEM = 1e-6 has over its own measurement (4.1e-7).
C_FUSED_MEASURED = 1.6e-7
C_FUSED = 2.4 * C_FUSED_MEASURED


def _fma32(acc, a, b):
    """fp32 fma (the product of two fp32 numbers is exact in fp64; the double rounding of the sum is rare and of no weight here)"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def emulate_fused(dXk, W, x0, Xp, Hp):
    """k_cin_bwd_fused's arithmetic on fp32 inputs: T by a c-ordered fma chain; dX_{k-1}: a chain over the fields of a parity (HP 64: the two
    parities joined), dx0: two-term partials per lane, a pairwise tree over the 32 lanes, the two wave columns joined (HP 128).  Returns the two
    contributions (rows, Hp), (rows, F) before they are added to the outputs."""
    R, Hk = dXk.shape
    F = x0.shape[1]
    T = np.zeros((R, F * Hp), np.float32)
    for cc in range(Hk):
        T = _fma32(T, dXk[:, cc:cc + 1], W[cc:cc + 1, :])
    T3 = T.reshape(R, F, Hp)
    G = 128 // Hp
    parts = []
    for par in range(G):
        acc = np.zeros((R, Hp), np.float32)
        for f in range(par, F, G):
            acc = _fma32(acc, T3[:, f], x0[:, f:f + 1])
        parts.append(acc)
    a = parts[0] if G == 1 else (parts[0] + parts[1]).astype(np.float32)
    b = np.zeros((R, F), np.float32)
    for f in range(F):
        tot = None
        for wn in range(Hp // 64):
            lo = 64 * wn
            pr = _fma32((T3[:, f, lo:lo + 32] * Xp[:, lo:lo + 32]).astype(np.float32), T3[:, f, lo + 32:lo + 64], Xp[:, lo + 32:lo + 64])
            n = 32
            while n > 1:
                n //= 2
                pr = (pr[:, :n] + pr[:, n:2 * n]).astype(np.float32)
            tot = pr[:, 0] if tot is None else (tot + pr[:, 0]).astype(np.float32)
        b[:, f] = tot
    return a, b


def fused_constant(Hk, Hp, F, rows=128, seed=0):
    """max over the elements of |emulate_fused - fp64| / sum |terms| on x ~ N(0, 0.5), W ~ U(-0.5, 0.5), dX ~ N(0, 1)"""
    rng = np.random.default_rng(seed + 1000 * Hk + 10 * Hp + F)
    dXk = rng.normal(0, 1, (rows, Hk)).astype(np.float32)
    W = rng.uniform(-0.5, 0.5, (Hk, F * Hp)).astype(np.float32)
    x0 = rng.normal(0, 0.5, (rows, F)).astype(np.float32)
    Xp = rng.normal(0, 0.5, (rows, Hp)).astype(np.float32)
    a, b = emulate_fused(dXk, W, x0, Xp, Hp)
    d = [v.astype(np.float64) for v in (dXk, W, x0, Xp)]
    T = (d[0] @ d[1]).reshape(rows, F, Hp)
    Ta = (np.abs(d[0]) @ np.abs(d[1])).reshape(rows, F, Hp)
    ra, ma = (T * d[2][:, :, None]).sum(1), (Ta * np.abs(d[2])[:, :, None]).sum(1)
    rb, mb = (T * d[3][:, None, :]).sum(2), (Ta * np.abs(d[3])[:, None, :]).sum(2)
    return max(float((np.abs(a - ra) / ma).max()), float((np.abs(b - rb) / mb).max()))

"""Integer census of a whole DCNMixLayer stack (csrc/dcnmix.hip, csrc/dcnmix_mid.hip, csrc/dcnmix_tile*.hip) and of its fused scoring head.

Every input is a small dyadic number, chosen so that every intermediate of the forward and the backward pass is an fp32 number and every sum the
kernels form -- a product over D, over S, over K = N S + N or over the batch, in any order, under any split-K, slab or per-workgroup partial --
keeps the sum of the absolute values of its terms below 2^24 units of their finest granularity.  A correct kernel then returns the exact value
to the bit; a kernel that drops a row block, doubles a partial, mixes up an expert or reads the wrong tensor does not.

Data (values from a per-element integer hash, tests/_exact_census.py `hash2`):
  x        nonzero integers in +-[1, xmax]
  U, V, W  sparse: `k` nonzero entries (+-1, +-2) per output column (U: per (n, s) over d; V: per (n, t) over s; W: per d over (n, s))
  K        one sparse column (+-1) repeated N times: every row's N gate logits are equal, so every softmax site computes exactly 1 / N
           (N in {1, 2, 4, 8}); a wrong column of the logit product breaks the equality
  b        integers in +-[1, 2]
  dy       +-1 on one row in `rho` (always the first and the last row of the batch and at least one row of every 32-row block), 0 elsewhere:
           the batch-deep weight-gradient sums stay inside the window at 25 600 rows.  dscores (score entry) likewise, head_w in +-{1, 2},
           head_b 1/2.
The activations are LINEAR or RELU (inner and outer); act' is taken from the stored output as the kernels do (rn_act_grad_from_out:
RELU'(y) = [y > 0]), so an exact-zero pre-activation gets the derivative 0 on both sides.

`make(B, D, S, N, L, head)` returns a Census whose parameters were shrunk (fewer nonzeros, smaller x, sparser dy) until every invariant holds
for both activations.  `restate(c, ai, ao, mm, mut)` is the layer in the kernels' factorisation, for any matrix product `mm` (fp64 exact,
fp32 in several summation orders) and with an optional planted mistake (MUTATIONS)."""
import numpy as np

from _exact_census import hash2, exact32, WINDOW

LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
ROWS = 32                       # rows of a workgroup's block (MID_ROWS, TL_ROWS)

# planted mistakes: name -> (what it models, applies(spec))
MUTATIONS = {
    'drop_last_row': ('the last row dropped from every weight-gradient sum', lambda s: True),
    'drop_last_block': ('the last 32-row block dropped from the weight-gradient sums (dV partials of the last workgroup)', lambda s: True),
    'dv_partial_twice': ("one workgroup's dV partial counted twice", lambda s: True),
    'wrong_expert_v': ("expert n reads expert n + 1's V", lambda s: s['N'] > 1),
    'bias_not_gated': ('the bias rows of the output product not weighted by the gate', lambda s: s['N'] > 1),
    'act_grad_wrong_tensor': ("act_outer' taken from H1 instead of H2, act_inner' from H2 instead of H1", lambda s: True),
    'xless_no_x0': ('the x0 multiply skipped in the x_l = x0 * O_{l-1} operand', lambda s: s['L'] > 1),
    'g_wrong_layer': ('the weight gradients dW, db of layer l formed with the gradient of the layer above (g_{l+2}) instead of g_{l+1}',
                      lambda s: s['L'] > 1),
    'head_db_missing': ('the head bias gradient left out', lambda s: s['head']),
}


def _sparse(shape, salt, k, vmax):
    """(cols_outer..., rows, cols) float64: per column (last axis) k nonzero entries in +-[1, vmax] at hashed rows (axis -2)."""
    nb, rows, cols = shape
    out = np.zeros(shape)
    pos = (hash2((nb, k, cols), salt) % np.uint64(rows)).astype(np.int64)          # (nb, k, cols)
    h = hash2((nb, k, cols), salt + 1)
    val = ((h % np.uint64(vmax)).astype(np.int64) + 1) * np.where((h >> np.uint64(40)) & np.uint64(1), -1, 1)
    for b in range(nb):
        for j in range(k):
            out[b, pos[b, j], np.arange(cols)] += val[b, j]
    return out


def _ints(shape, salt, vmax):
    h = hash2(shape, salt)
    return (((h % np.uint64(vmax)).astype(np.int64) + 1) * np.where((h >> np.uint64(40)) & np.uint64(1), -1, 1)).astype(np.float64)


def grad_rows(B, rho, salt):
    """rows with a nonzero upstream gradient: one in rho (hashed), the first and last row, and one row in every 32-row block"""
    h = hash2((1, B, 1), salt)[0, :, 0]
    on = (h % np.uint64(rho)) == 0
    on[0] = on[-1] = True
    blk = np.arange(0, B, ROWS)
    on[np.minimum(blk + (hash2((1, len(blk), 1), salt + 7)[0, :, 0] % np.uint64(ROWS)).astype(np.int64), B - 1)] = True
    return on


class Census:
    """spec: B, D, S, N, L, head.  params: (k, xmax, rho) of the data.  inp: float32 arrays x (B, D), U[l] (N, D, S), V[l] (N, S, S),
    W[l] (N, S, D), b[l] (N, D), K[l] (D, N), dy (B, D) or ds (B,), hw (D,), hb (1,)."""


def _inputs(s, k, xmax, rho):
    B, D, S, N, L = s['B'], s['D'], s['S'], s['N'], s['L']
    inp = {'x': _ints((1, B, D), 3, xmax)[0]}
    for key in ('U', 'V', 'W', 'b', 'K'):
        inp[key] = []
    for l in range(L):
        base = 100 * (l + 1)
        inp['U'].append(_sparse((N, D, S), base + 1, k, 2))
        inp['V'].append(_sparse((N, S, S), base + 3, k, 1))
        Wc = _sparse((1, N * S, D), base + 5, k, 2)[0]
        inp['W'].append(Wc.reshape(N, S, D))
        inp['b'].append(_ints((1, N, D), base + 7, 2)[0])
        col = _sparse((1, D, 1), base + 9, 2, 1)[0]
        inp['K'].append(np.repeat(col, N, axis=1))
    on = grad_rows(B, rho, 11)
    if s['head']:
        inp['ds'] = _ints((1, B, 1), 13, 1)[0, :, 0] * on
        inp['hw'] = _ints((1, 1, D), 17, 2)[0, 0]
        inp['hb'] = np.array([0.5])
    else:
        inp['dy'] = _ints((1, B, D), 13, 1)[0] * on[:, None]
    return inp


def act(v, a):
    if a == TANH:
        return np.tanh(v)
    if a == SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v if a == LINEAR else np.where(v > 0, v, 0.0)


def act_grad(y, a):
    """rn_act_grad_from_out: the derivative from the activation's OUTPUT"""
    if a == TANH:
        return 1.0 - y * y
    if a == SIGMOID:
        return y * (1.0 - y)
    return np.ones_like(y) if a == LINEAR else (y > 0).astype(y.dtype)


def _frac_bits(x):
    """smallest f >= 0 with x * 2^f integral for every element (dyadic x; fp64 significands)"""
    m, e = np.frexp(x[x != 0].astype(np.float64))
    if m.size == 0:
        return 0
    v = np.abs(np.ldexp(m, 53)).astype(np.int64)
    tz = np.log2((v & -v).astype(np.float64)).astype(np.int64)      # trailing zero bits of the 53-bit significand
    return int(max(0, (53 - tz - e).max()))


def mm64(A, B):
    return A @ B


def _bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32; finite inputs well inside the bf16 range"""
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split3(x):
    """the three bf16 pieces of fp32 x, round to nearest even each (tests/_split_census.py bf16_split, vectorised in numpy)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p1 = _bf16_rne(x)
    r = x - p1
    p2 = _bf16_rne(r)
    return p1, p2, _bf16_rne(r - p2)


def _split_abs(A):
    """(|p1| + |p2| elementwise, count of nonzero third pieces) of the bf16x3 split of fp32 A"""
    p1, p2, p3 = split3(A)
    return np.abs(p1.astype(np.float64)) + np.abs(p2.astype(np.float64)), int(np.count_nonzero(p3))


class Tracker:
    """Records, for every product, the worst sum of |terms| in units of the finest term granularity, plain and in the bf16x3 split form."""

    def __init__(self):
        self.split_units = {}
        self.bits = {}

    def __call__(self, name, A, B):
        C = A @ B
        if A.size and B.size and np.any(A) and np.any(B):
            fa, fb = _frac_bits(A), _frac_bits(B)
            sa, ta = _split_abs(A)
            sb, tb = _split_abs(B)
            self.bits[name] = self.bits.get(name, 0) + ta + tb
            su = float((sa @ sb).max()) * 2.0 ** (fa + fb)         # >= the plain sum of |terms| (|a1| + |a2| >= |a|)
            self.split_units[name] = max(self.split_units.get(name, 0.0), su)
            if su >= WINDOW:
                raise AssertionError('%s: sum of |terms| %d units >= 2^24' % (name, su))
        return C


def restate(c, ai, ao, mm=mm64, mut=None, dtype=np.float64, keep=False):
    """The layer stack (+ head) forward and backward in the kernels' factorisation.  mm(name, A, B) or mm(A, B): the product.  Returns the
    checked outputs (and, with keep, every intermediate).  dtype: the arithmetic of the elementwise steps."""
    s = c.spec
    B, D, S, N, L = s['B'], s['D'], s['S'], s['N'], s['L']
    NS = N * S
    f = lambda a: np.asarray(a, dtype=dtype)     # noqa: E731
    P = (lambda name, A, Bm: mm(name, A, Bm)) if isinstance(mm, Tracker) else (lambda name, A, Bm: mm(A, Bm))
    inp = {k: ([f(v) for v in vv] if isinstance(vv, list) else f(vv)) for k, vv in c.inp.items()}
    x0 = inp['x']
    Uc = [u.transpose(1, 0, 2).reshape(D, NS) for u in inp['U']]             # [U_0 | .. | U_{N-1}] (D, NS)
    Vs = inp['V']
    if mut == 'wrong_expert_v':
        Vs = [np.roll(v, -1, axis=0) for v in Vs]
    Wb = [np.concatenate([w.reshape(NS, D), b], 0) for w, b in zip(inp['W'], inp['b'])]      # [W; b] (NS + N, D)
    out, keepd = {}, {'T1': [], 'H2': [], 'O': [], 'x': [x0]}
    xl = x0
    fw = []
    for l in range(L):
        xin = xl
        if mut == 'xless_no_x0' and l > 0:
            xin = keepd['O'][l - 1]
        Z = P('x_l U', xin, Uc[l])
        lg = P('x_l K', xin, inp['K'][l])
        H1 = act(Z, ai)
        C = np.concatenate([P('H1 V', H1[:, n * S:(n + 1) * S], Vs[l][n]) for n in range(N)], 1)
        H2 = act(C, ao)
        e = np.exp(lg - lg.max(1, keepdims=True))
        G = (e / e.sum(1, keepdims=True)).astype(dtype)
        Ge = np.repeat(G, S, axis=1)
        T2g = Ge * H2
        Tg = np.concatenate([T2g, G if mut != 'bias_not_gated' else np.ones_like(G)], 1)
        O = P('T2g [W; b]', Tg, Wb[l])
        xn = x0 * O
        fw.append(dict(xl=xin, H1=H1, H2=H2, G=G, T2g=T2g, O=O))
        keepd['T1'].append(np.concatenate([H1, lg], 1))
        keepd['H2'].append(H2)
        keepd['O'].append(O)
        keepd['x'].append(xn)
        xl = xn
    y = xl
    if s['head']:
        hw = inp['hw']
        out['scores'] = P('y w_head', y, hw[:, None])[:, 0] + inp['hb'][0]
    else:
        out['y'] = y
    # ---- backward
    rows = np.ones(B, bool)
    if mut == 'drop_last_row':
        rows[-1] = False
    if mut == 'drop_last_block':
        rows[-ROWS:] = False
    r = rows[:, None].astype(dtype)

    def wgrad(name, A, Bm):      # a K = B product (weight gradient): sum over the kept rows
        return P(name, (A * r).T, Bm)
    g = None if s['head'] else inp['dy']
    g_above = None               # g of the layer above (mutation g_wrong_layer)
    dx_terms = []
    track = isinstance(mm, Tracker)
    for l in range(L - 1, -1, -1):
        st = fw[l]
        top_head = s['head'] and l == L - 1
        if top_head:             # dy = ds (x) w_head is never stored: dT2g = ds * (x (W w_head)^T)
            ds, hw = inp['ds'], inp['hw']
            dTg = ds[:, None] * P('x (W w_head)^T', x0, (Wb[l] * hw[None, :]).T)
            g = ds[:, None] * hw[None, :]
            if track:            # the row-block kernels' factorisation: (x dy) [W; b]^T
                P('(x g) [W; b]^T', x0 * g, Wb[l].T)
        else:
            dTg = P('(x g) [W; b]^T', x0 * g, Wb[l].T)
        g_w = g_above if (mut == 'g_wrong_layer' and g_above is not None) else g
        H1, H2, G, T2g = st['H1'], st['H2'], st['G'], st['T2g']
        dT2g, dG_side = dTg[:, :NS], dTg[:, NS:]
        Ge = np.repeat(G, S, axis=1)
        dG = np.stack([P('dT2g H2 row dot', dT2g[:, n * S:(n + 1) * S] * H2[:, n * S:(n + 1) * S], np.ones((S, 1), dtype))[:, 0]
                       for n in range(N)], 1) + dG_side
        dot = P('<G, dG>', G * dG, np.ones((N, 1), dtype))
        dlog = G * (dG - dot)
        dC = Ge * dT2g * act_grad(H1 if mut == 'act_grad_wrong_tensor' else H2, ao)
        dV, dH1 = [], []
        for n in range(N):
            sl = slice(n * S, (n + 1) * S)
            v = wgrad('H1^T dC', H1[:, sl], dC[:, sl])
            if mut == 'dv_partial_twice':
                v = v + P('H1^T dC', H1[:ROWS, sl].T, dC[:ROWS, sl])
            dV.append(v)
            dH1.append(P('dC V^T', dC[:, sl], Vs[l][n].T))
        dA = np.concatenate(dH1, 1) * act_grad(H2 if mut == 'act_grad_wrong_tensor' else H1, ai)
        gprev = P('[dA | dlogits] [U | K]^T', np.concatenate([dA, dlog], 1), np.concatenate([Uc[l], inp['K'][l]], 1).T)
        TgG = np.concatenate([T2g, G], 1)
        if top_head:             # M = x^T (ds [T2g | G]); dW = w_head M^T; d w_head[c] = sum_k [W; b][k][c] M[c][k]
            M = wgrad('x^T (ds T2g)', x0, ds[:, None] * TgG)
            dWb = (M * hw[:, None]).T
            out['dhead_w'] = P('[W; b] M^T row dot', Wb[l].T * M, np.ones((NS + N, 1), dtype))[:, 0]
            out['dhead_b'] = np.zeros(1, dtype) if mut == 'head_db_missing' else P('sum ds', (ds * rows)[None, :], np.ones((B, 1), dtype))[0]
            if track:
                wgrad('(x g)^T [T2g | G]', x0 * g, TgG)
                P('y^T ds', (y * r).T, ds[:, None])
        else:
            dWb = wgrad('(x g)^T [T2g | G]', x0 * g_w, TgG).T
        out['dW%d' % l] = dWb[:NS].reshape(N, S, D)
        out['db%d' % l] = dWb[NS:]
        out['dV%d' % l] = np.stack(dV)
        out['dU%d' % l] = wgrad('x_l^T dA', st['xl'], dA).reshape(D, N, S).transpose(1, 0, 2)
        out['dK%d' % l] = wgrad('x_l^T dlogits', st['xl'], dlog)
        if s['need_dx']:
            dx_terms.append(g * st['O'])       # x_{l+1} = x0 * O_l
            if l == 0:
                dx_terms.append(gprev)         # g_0
        keepd.setdefault('g', []).append(gprev)
        g_above, g = g, gprev
    if s['need_dx']:
        t = np.stack(dx_terms)
        out['dx'] = P('dx terms', t.reshape(len(dx_terms), -1).T, np.ones((len(dx_terms), 1), dtype))[:, 0].reshape(B, D)
    if keep:
        out['_keep'] = keepd
        out['_fw'] = fw
    return out


def check_intermediates(c, ai, ao):
    """Every intermediate of the stack is an fp32 number and has at most 16 significant bits (the third bf16 piece is zero)."""
    res = restate(c, ai, ao, keep=True)
    k = res['_keep']
    arrays = [('x%d' % i, v) for i, v in enumerate(k['x'])] + [('T1', v) for v in k['T1']] + [('H2', v) for v in k['H2']] + \
             [('O', v) for v in k['O']] + [('g', v) for v in k.get('g', [])]
    arrays += [(n, v) for n, v in res.items() if not n.startswith('_')]
    for name, v in arrays:
        assert exact32(v).all(), '%s is not an fp32 number' % name
    for name, v in arrays[:-len([n for n in res if not n.startswith('_')])]:
        assert _split_abs(v)[1] == 0, '%s has more than 16 significant bits' % name
    return res


def units(c, ai, ao):
    t = Tracker()
    restate(c, ai, ao, mm=t)
    return t


# (k nonzeros per weight column, xmax, one row in rho carries a gradient; rho grows with the batch beyond 1024 rows)
LADDER = ((2, 2, 8), (2, 2, 32), (1, 2, 16), (1, 2, 64), (1, 1, 64), (1, 1, 256))


def make(B, D, S, N, L, head=False, need_dx=True, params=None, verify=True):
    """A census of the stack (see the module docstring).  params (k, xmax, rho) or None: the first LADDER entry for which every invariant holds
    for LINEAR and RELU (rho scaled by B / 1024 beyond 1024 rows).  verify=False: take `params` as they are (checked by the CPU census test)."""
    assert N in (1, 2, 4, 8)
    spec = dict(B=B, D=D, S=S, N=N, L=L, head=bool(head), need_dx=bool(need_dx))
    last = None
    for p in ([params] if params is not None else LADDER):
        k, xmax, rho = p
        c = Census()
        c.spec, c.params = spec, tuple(p)
        c.inp = {kk: ([a.astype(np.float32) for a in v] if isinstance(v, list) else v.astype(np.float32))
                 for kk, v in _inputs(spec, k, xmax, rho * max(1, B // 1024)).items()}
        if not verify:
            return c
        try:
            for ai, ao in ((LINEAR, LINEAR), (RELU, RELU)):
                t = units(c, ai, ao)
                worst = max(t.split_units.values())
                assert worst < WINDOW, 'sum of |terms| %d units >= 2^24 (%s)' % (worst, max(t.split_units, key=t.split_units.get))
                assert not any(t.bits.values()), 'an operand with more than 16 significant bits: %r' % {n: v for n, v in t.bits.items() if v}
                check_intermediates(c, ai, ao)
        except AssertionError as e:
            last = e
            continue
        return c
    raise AssertionError('no census parameters keep %r exact: %s' % (spec, last))


def expected(c, ai, ao):
    """The exact outputs (fp64): scores or y, dx (need_dx), dU_l, dV_l, dW_l, db_l, dK_l, dhead_w / dhead_b (head)."""
    return restate(c, ai, ao)


# ---- fp32 restatements in several summation orders -------------------------------------------------------------------------------------
def mm32_plain(A, B):
    return np.matmul(A.astype(np.float32), B.astype(np.float32))


def mm32_reversed(A, B):
    return np.matmul(A[:, ::-1].astype(np.float32), B[::-1].astype(np.float32))


def mm32_blocked(A, B, blk=32):
    """split-K in blocks of `blk` (the workgroup partials), the partials added last block first, one fp32 add at a time"""
    A, B = A.astype(np.float32), B.astype(np.float32)
    K = A.shape[1]
    acc = None
    for k0 in reversed(range(0, K, blk)):
        p = np.matmul(A[:, k0:k0 + blk], B[k0:k0 + blk])
        acc = p if acc is None else (acc + p).astype(np.float32)
    return acc


ORDERS = {'plain': mm32_plain, 'reversed': mm32_reversed, 'blocked': mm32_blocked}

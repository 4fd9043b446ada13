"""Integer census of the exact-fp32 products (csrc/gemm.hip rn_gemm_impl, every k_gemm instantiation of csrc/gemm_inst_*.hip).

On gfx950 an fp32 MFMA is a k-ordered chain of fp32 fmaf.  If every operand is a small dyadic number and, for every output, the sum of the
absolute values of its terms stays below 2^24 units of the finest granularity, then every partial sum of every order, tiling and K split is an
fp32 number: the correct kernel returns the fp64 product to the bit.  A kernel that drops a k-tile, shifts a row, reads the bias of the
neighbouring column or mixes up an operand kind does not.

Operands (values from a per-element integer hash, so neighbouring rows, columns and k differ):
  A, B               nonzero integers in +-[1, vmax] (vmax 7, shrunk to 3 or 1 where the 2^24 invariant would not hold)
  MUL second         integers in +-[1, 3]
  ACTGRAD second     outputs y with an exact dyadic act'(y) = rn_act_grad_from_out(y, act), contracted to an fma or not:
                     RELU y in {-1, 0, 1, 2}; TANH y = j / 8 (1 - y^2, |j| <= 7); SIGMOID y = j / 16 (y (1 - y), 1 <= j <= 15)
  OUTER pair         stored(r, c) = second[r][c / hq] * first[r][c % hq] on the STORED layout of the operand (include/recnow.h)
  bias, C0           multiples of 1/4 in +-[1/4, 15/4];  emul MUL: +-2^{-1, 0, 1};  emul ACTGRAD: y as above
  Bx, P, Q, as_in    integers in +-[1, 3]
Every epilogue step (bias, rank-R update, activation, emul, accumulate) is checked to be exact in fp32, in the kernel's order.

`make(spec)` returns a Census: the stored operands (logical elements only, float32, per batch), the effective operands A' (M, K) and B' (K, N)
in fp64, and `expected(act)` the exact C, Cx and as_out.
"""
import numpy as np

WINDOW = 1 << 24          # fp32 significand: partial sums below 2^24 units are exact in any order
LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
NONE, MUL, ACTGRAD, OUTER = 0, 1, 2, 3

SPEC_DEFAULTS = dict(M=128, N=128, K=128, batch=1, ta=0, tb=0, a_mode=0, b_mode=0, a_act=TANH, b_act=SIGMOID, a_hq=0, b_hq=0, sp_r=0, eu_r=0,
                     as_out=0, bias=0, e_mode=0, e_act=RELU, accumulate=0, act_cols=0, k_valid=0, c_trans=0)


def _mix(x):
    x = x ^ (x >> np.uint64(31))
    x = x * np.uint64(0x7FB5D329728EA185)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x81DADEF4BC2DD44D)
    return x ^ (x >> np.uint64(33))


def hash2(shape, salt):
    """uint64 hash of (batch, row, col, salt) for an array of `shape` (batch, rows, cols)."""
    b, r, c = (np.arange(n, dtype=np.uint64) for n in shape)
    with np.errstate(over='ignore'):
        x = (b[:, None, None] * np.uint64(0x9E3779B97F4A7C15) + r[None, :, None] * np.uint64(0xBF58476D1CE4E5B9) +
             c[None, None, :] * np.uint64(0x94D049BB133111EB) + np.uint64(salt) * np.uint64(0xD6E8FEB86659FD93))
        return _mix(_mix(x))


def ints(shape, salt, vmax):
    """Nonzero integers in +-[1, vmax], float64."""
    h = hash2(shape, salt)
    mag = (h % np.uint64(vmax)).astype(np.int64) + 1
    sign = np.where((h >> np.uint64(40)) & np.uint64(1), -1, 1)
    return (sign * mag).astype(np.float64)


def actgrad_outputs(shape, salt, act):
    """Stored `y` of an ACTGRAD operand whose factor rn_act_grad_from_out(y, act) is exact."""
    h = hash2(shape, salt)
    if act == RELU:
        return (h % np.uint64(4)).astype(np.float64) - 1.0                      # -1, 0, 1, 2
    if act == TANH:
        return ((h % np.uint64(15)).astype(np.float64) - 7.0) / 8.0             # -7/8 .. 7/8
    if act == SIGMOID:
        return ((h % np.uint64(15)).astype(np.float64) + 1.0) / 16.0            # 1/16 .. 15/16
    raise ValueError(act)


def act_grad(y, act):
    """rn_act_grad_from_out in fp64 (exact for the census's y)."""
    return [np.ones_like(y), (y > 0).astype(np.float64), 1.0 - y * y, y * (1.0 - y)][act]


def act64(v, act):
    with np.errstate(over='ignore', invalid='ignore'):
        return [v, np.where(v > 0, v, 0.0), np.tanh(v), 1.0 / (1.0 + np.exp(-v))][act]


def exact32(x):
    """True where x (fp64) is exactly an fp32 number (non-finite values count as exact)."""
    with np.errstate(over='ignore', invalid='ignore'):
        return (x.astype(np.float32).astype(np.float64) == x) | ~np.isfinite(x)


def frac_bits(x):
    """Smallest f >= 0 with x * 2^f integral for every element (dyadic x)."""
    x = np.abs(x[np.isfinite(x)])
    for f in range(0, 64):
        y = x * 2.0 ** f
        if np.array_equal(y, np.floor(y)):
            return f
    raise AssertionError('operand is not dyadic')


class Census:
    """stored: name -> float32 (batch, rows, cols) logical arrays in the layout the kernel reads (A, A2, B, B2, bias (batch, 1, N),
    E, C0, Bx (1, K, sp_r), P (1, M, eu_r), Q (1, eu_r, N), as_in (1, rows, cols)).  Ae (batch, M, K), Be (batch, K, N): effective
    operands in fp64.  units: log2 of the finest granularity of the terms."""


def effective(spec, st, side):
    """The effective operand (batch, M, K) for side 'A' / (batch, K, N) for 'B' from the stored arrays, in fp64 (non-finite values propagate)."""
    s = spec
    first = st[side].astype(np.float64)
    mode = s['a_mode'] if side == 'A' else s['b_mode']
    with np.errstate(over='ignore', invalid='ignore'):
        if mode == MUL:
            v = first * st[side + '2']
        elif mode == ACTGRAD:
            v = first * act_grad(st[side + '2'].astype(np.float64), s['a_act'] if side == 'A' else s['b_act'])
        elif mode == OUTER:
            hq = s['a_hq'] if side == 'A' else s['b_hq']
            cols = st[side + '2'].shape[2] * hq
            c = np.arange(cols)
            v = st[side + '2'].astype(np.float64)[:, :, c // hq] * first[:, :, c % hq]
        else:
            v = first
    trans = s['ta'] if side == 'A' else s['tb']               # stored [K][M] for A, [N][K] for B: transpose to the logical layout
    return np.ascontiguousarray(v.transpose(0, 2, 1)) if trans else v


def stored_shape(spec, side):
    s = spec
    if side == 'A':
        return (s['K'], s['M']) if s['ta'] else (s['M'], s['K'])
    return (s['N'], s['K']) if s['tb'] else (s['K'], s['N'])


def _operands(s, vmax):
    st = {}
    for side, salt in (('A', 11), ('B', 23)):
        rows, cols = stored_shape(s, side)
        mode = s['a_mode'] if side == 'A' else s['b_mode']
        nb = s['batch'] if mode != OUTER else 1
        if mode == OUTER:
            hq = s['a_hq'] if side == 'A' else s['b_hq']
            assert cols % hq == 0
            st[side] = ints((nb, rows, hq), salt, vmax)
            st[side + '2'] = ints((nb, rows, cols // hq), salt + 1, 3)
        else:
            st[side] = ints((nb, rows, cols), salt, vmax)
            if mode == MUL:
                st[side + '2'] = ints((nb, rows, cols), salt + 1, 3)
            elif mode == ACTGRAD:
                st[side + '2'] = actgrad_outputs((nb, rows, cols), salt + 1, s['a_act'] if side == 'A' else s['b_act'])
        if s['k_valid']:                                      # a depth padded with zeros: the operands' k >= k_valid are 0
            kv = s['k_valid']
            kax = (1 if s['ta'] else 2) if side == 'A' else (2 if s['tb'] else 1)
            sl = [slice(None)] * 3
            sl[kax] = slice(kv, None)
            st[side][tuple(sl)] = 0.0
    M, N, K, nb = s['M'], s['N'], s['K'], s['batch']
    if s['bias']:
        st['bias'] = ints((nb, 1, N), 31, 15) / 4.0
    if s['e_mode'] == MUL:
        st['E'] = np.ldexp(np.sign(ints((nb, M, N), 37, 1)), (hash2((nb, M, N), 38) % np.uint64(3)).astype(np.int64) - 1)
    elif s['e_mode'] == ACTGRAD:
        st['E'] = actgrad_outputs((nb, M, N), 37, s['e_act'])
    if s['accumulate']:
        st['C0'] = ints((nb, M, N), 41, 15) / 4.0
    if s['sp_r']:
        st['Bx'] = ints((1, K, s['sp_r']), 43, 3)
    if s['eu_r']:
        st['P'] = ints((1, M, s['eu_r']), 47, 3)
        st['Q'] = ints((1, s['eu_r'], N), 53, 3)
    if s['as_out']:
        st['as_in'] = ints((1,) + stored_shape(s, 'A'), 59, 3)
    return st


def make(spec=None, **kw):
    """A census of one product (see the module docstring).  The value range shrinks (vmax 7 -> 3 -> 1) until every invariant holds."""
    s = dict(SPEC_DEFAULTS)
    s.update(spec or {})
    s.update(kw)
    last = None
    for vmax in (7, 3, 1):
        st = _operands(s, vmax)
        c = Census()
        c.spec, c.vmax, c.stored = s, vmax, {k: v.astype(np.float32) for k, v in st.items()}
        assert all(np.array_equal(v.astype(np.float32).astype(np.float64), v) for v in st.values())
        c.Ae, c.Be = effective(s, st, 'A'), effective(s, st, 'B')
        if s['as_out']:
            assert s['a_mode'] == MUL
        try:
            check_invariants(c)
        except AssertionError as e:
            last = e
            continue
        return c
    raise AssertionError('no census value range keeps %r exact: %s' % (s, last))


def term_units(c):
    """max over outputs of sum_k |A'_ik B'_kj| (+ the rank-R terms), in units of the finest term granularity; and that granularity's log2."""
    fa, fb = frac_bits(c.Ae), frac_bits(c.Be)
    mag = np.abs(c.Ae) @ np.abs(c.Be)
    if c.spec['eu_r']:
        mag = mag + np.abs(c.stored['P'].astype(np.float64)) @ np.abs(c.stored['Q'].astype(np.float64))
    worst = float(mag.max()) * 2.0 ** (fa + fb)
    if c.spec['sp_r']:
        worst = max(worst, float((np.abs(c.Ae[0]) @ np.abs(c.stored['Bx'][0].astype(np.float64))).max()) * 2.0 ** fa)
    return worst, fa + fb


def check_invariants(c):
    """The exactness invariant of the product and the fp32 exactness of every epilogue step (LINEAR and RELU)."""
    worst, _ = term_units(c)
    assert worst < WINDOW, 'sum of |terms| = %d units >= 2^24' % worst
    for act in (LINEAR, RELU):
        expected(c, act, check=True)


def preactivation(c, check=False):
    """z = A' B' + bias (+ rank-R update), fp64 (exact), with the kernel's order of operations checked for fp32 exactness."""
    z = c.Ae @ c.Be
    steps = [z]
    if c.spec['bias']:
        z = z + c.stored['bias'].astype(np.float64)
        steps.append(z)
    if c.spec['eu_r']:
        z = z + c.stored['P'][0].astype(np.float64) @ c.stored['Q'][0].astype(np.float64)
        steps.append(z)
    if check:
        for v in steps:
            assert exact32(v).all(), 'an epilogue step before the activation is not exact in fp32'
    return z


def finish(c, v, check=False):
    """The epilogue after the activation: emul, accumulate (fp64, exact for census inputs when `check` passes)."""
    s = c.spec
    if s['e_mode']:
        E = c.stored['E'].astype(np.float64)
        v = v * (E if s['e_mode'] == MUL else act_grad(E, s['e_act']))
        if check:
            assert exact32(v).all(), 'emul step not exact in fp32'
    if s['accumulate']:
        v = v + c.stored['C0'].astype(np.float64)
        if check:
            assert exact32(v).all(), 'accumulate step not exact in fp32'
    return v


def apply_act(c, z, act):
    cols = c.spec['act_cols'] or c.spec['N']
    out = z.copy()
    out[..., :cols] = act64(z[..., :cols], act)
    return out


def expected(c, act=LINEAR, check=False):
    """(C (batch, M, N), Cx (M, sp_r) or None, as_out (stored A layout) or None), fp64; exact for LINEAR / RELU."""
    z = preactivation(c, check)
    C = finish(c, apply_act(c, z, act), check)
    Cx = c.Ae[0] @ c.stored['Bx'][0].astype(np.float64) if c.spec['sp_r'] else None
    aso = c.stored['A'][0].astype(np.float64) * c.stored['as_in'][0] if c.spec['as_out'] else None
    if check:
        for v in (C, Cx, aso):
            assert v is None or exact32(v).all(), 'an output is not an fp32 number'
    return C, Cx, aso


def permute_store(C, s):
    """The c_perm_s layout of a (M, N) result: flat [N / s][M][s]."""
    M, N = C.shape
    return C.reshape(M, N // s, s).transpose(1, 0, 2).reshape(-1)

"""The route table of MultiDense (csrc/layers.hip recnow_multi_dense_fwd / _bwd): one row per kernel family, instance, grid cap and boundary, with
the call that reaches it.  Used by tests/test_dense_routes_gpu.py (on the GPU) and tests/test_dense_routes_cpu.py (the table agrees with the
predicates restated here, covers every instance and boundary, and its integer data is exact in fp32).

How a call picks its kernels (csrc/layers.hip):
  head_ok    N = 1, U = 1, D % 4 = 0, 64 <= D <= 4096, x and kernel 16-byte aligned (backward: dx too, when requested):
             k_head_fwd<1 | 4 | 16> (D <= 256 | <= 1024 | else; at most 2048 workgroups of 4 rows, two rows per step), k_head_dw_partial (chunks of
             HEAD_ROWS = 128 rows, 8 rows per step) + column sum, k_head_dx (at most 8192 workgroups), dbias = column sum of dZ
  narrow_ok  N = 1, B >= 4096, D % 4 = 0, U % 4 = 0, D <= 128, U <= 128, D U <= 4096: k_narrow_dense<NO / 4> for y (NO = U) and for dx (NO = D),
             tiles of ND_ROWS = 64 rows on at most 2048 workgroups
  xty_ok     N = 1, B >= 4096, D <= 128, U <= 128, D U / 256 in {1, 2, 4, 8, 16} (and U a multiple of it): k_small_xty<D U / 256> for dkernel, with
             dbias from the same pass; at most 1024 workgroups of >= 128 rows
  bias sums  N > 1 and U >= 64: rn_colsum_batched (all experts in one pair of launches); else one rn_colsum per expert
  dx         x broadcast to the N experts (x_batched = 0): one product per expert, accumulated in order; batched x: one batched product
  else       rn_gemm (csrc/gemm.hip).  The three predicates are independent: y / dx, dkernel and dbias of one call can take different families.
  B = 0      no launch; the backward zeroes dkernel and dbias

What the GPU test can prove: every rn_gemm launch records one GEMM-family tag (csrc/prof.hpp), the head, narrow and register-tile kernels and
the column sums record none.  So the number of GEMM tags of the forward call and of the backward call must equal the row's `gemm_fwd` /
`gemm_bwd`.  Rows whose difference from a neighbour has no tag -- WHICH k_head_fwd / k_small_xty instance ran, batched or per-expert bias sums,
a grid cap -- are proven only through their results on integer data (bit for bit) and say so in `why` ("no tag: ...").

Row fields: name, why, B, D, U, N, x_batched, want (subset of 'dx', 'dkernel', 'dbias'), x_off / dx_off (pointer offsets in floats), and the
declared routes y, dkernel, dbias, dx (strings below)."""

HEAD_ROWS, ND_ROWS, XTY_CAP_ROWS = 128, 64, 1024 * 128
HEAD_FWD_CAP_ROWS = 2 * 2048 * 4          # rows of one trip of k_head_fwd's loop at its 2048-workgroup cap (two rows per wave and step)
HEAD_DX_CAP_QUADS = 8192 * 256            # float4 stores of one trip of k_head_dx's loop at its 8192-workgroup cap
NARROW_CAP_ROWS = 2048 * ND_ROWS
NARROW_MIN_B = 4096

GEMM_TAGS = frozenset((1, 2, 3, 4, 5, 8, 9, 12))      # csrc/prof.hpp RN_TAG_GEMM_*: every rn_gemm launch records exactly one of them

ROUTES = []


def head_ok(D, U, N, x_off=0, dx_off=0, want_dx=False):
    return N == 1 and U == 1 and D % 4 == 0 and 64 <= D <= 4096 and x_off % 4 == 0 and (not want_dx or dx_off % 4 == 0)


def narrow_ok(B, D, U, N):
    return N == 1 and B >= NARROW_MIN_B and D % 4 == 0 and U % 4 == 0 and D <= 128 and U <= 128 and D * U <= 4096


def xty_ok(B, D, U, N):
    du = D * U
    if not (N == 1 and B >= NARROW_MIN_B and D <= 128 and U <= 128 and du % 256 == 0):
        return False
    nq = du // 256
    return nq in (1, 2, 4, 8, 16) and U % nq == 0


def bias_batched(U, N):
    return N > 1 and U >= 64


def predicted(r):
    """{'y', 'dkernel', 'dbias', 'dx', 'gemm_fwd', 'gemm_bwd'} of a row, from the predicates above"""
    B, D, U, N = r['B'], r['D'], r['U'], r['N']
    want = r['want']
    if B == 0:
        return dict(y='none', dkernel='zero' if 'dkernel' in want else 'none', dbias='zero' if 'dbias' in want else 'none', dx='none',
                    gemm_fwd=0, gemm_bwd=0)
    out = {}
    if head_ok(D, U, N, r['x_off']):
        out['y'] = 'head_fwd<%d>' % (1 if D <= 256 else 4 if D <= 1024 else 16)
    elif narrow_ok(B, D, U, N):
        out['y'] = 'narrow'
    else:
        out['y'] = 'gemm'
    out['gemm_fwd'] = int(out['y'] == 'gemm')
    if head_ok(D, U, N, r['x_off'], r['dx_off'], 'dx' in want):
        out.update(dkernel='head_dw' if 'dkernel' in want else 'none', dx='head_dx' if 'dx' in want else 'none',
                   dbias='colsum' if 'dbias' in want else 'none', gemm_bwd=0)
        return out
    g = 0
    xty = 'dkernel' in want and xty_ok(B, D, U, N)
    if 'dkernel' not in want:
        out['dkernel'] = 'none'
    elif xty:
        out['dkernel'] = 'xty<%d>' % (D * U // 256)
    else:
        out['dkernel'] = 'gemm'
        g += 1
    if 'dbias' not in want:
        out['dbias'] = 'none'
    elif xty:
        out['dbias'] = 'xty_fused'
    else:
        out['dbias'] = 'colsum_batched' if bias_batched(U, N) else 'colsum'
    if 'dx' not in want:
        out['dx'] = 'none'
    elif narrow_ok(B, D, U, N):
        out['dx'] = 'narrow'
    elif r['x_batched']:
        out['dx'] = 'gemm_batched'
        g += 1
    else:
        out['dx'] = 'gemm_bcast'
        g += N
    out['gemm_bwd'] = g
    return out


ALL = ('dx', 'dkernel', 'dbias')


def row(name, why, B, D, U, N=1, xb=0, want=ALL, x_off=0, dx_off=0, y='gemm', dkernel='gemm', dbias='colsum', dx='gemm_bcast'):
    r = dict(name=name, why=why, B=B, D=D, U=U, N=N, x_batched=xb, want=tuple(want), x_off=x_off, dx_off=dx_off, y=y, dkernel=dkernel, dbias=dbias,
             dx=dx)
    r['gemm_fwd'] = int(y == 'gemm')
    r['gemm_bwd'] = int(dkernel == 'gemm') + (1 if dx == 'gemm_batched' else N if dx == 'gemm_bcast' else 0)
    ROUTES.append(r)


def _head(name, why, B, D, nv, dkernel='head_dw', dbias='colsum', dx='head_dx', **kw):
    row(name, why, B, D, 1, y='head_fwd<%d>' % nv, dkernel=dkernel, dbias=dbias, dx=dx, **kw)


# ---- scoring head ------------------------------------------------------------------------------------------------------------------------------
_head('head_d64_b5', 'D = 64, the lower edge of head_ok; B = 5: two workgroups, no wave has a second row.  no tag: NV = 1 instance', 5, 64, 1)
_head('head_d256_b9', 'D = 256, the last width of k_head_fwd<1> (every lane holds one float4); B = 9: no second row', 9, 256, 1)
_head('head_d260_b131', 'D = 260, the first width of k_head_fwd<4> (one lane of the second float4 column); B = 131: the second chunk of '
      'k_head_dw_partial holds three remainder rows only; 33 workgroups, no second row.  no tag: NV = 4',
      131, 260, 4)
_head('head_d1024_b139', 'D = 1024, the last width of k_head_fwd<4>; B = 139: the second chunk of k_head_dw_partial is one 8-row block plus three '
      'remainder rows', 139, 1024, 4)
_head('head_d1028_b9', 'D = 1028, the first width of k_head_fwd<16>.  no tag: NV = 16', 9, 1028, 16)
_head('head_d4096_b2049', 'D = 4096, the upper edge of head_ok (k_head_dw_partial: four column trips per thread); B D / 4 = 2049 x 1024 > 8192 x 256: '
      'k_head_dx at its workgroup cap, some threads store a second float4.  no tag: the cap', 2049, 4096, 16)
_head('head_stride_b16389', 'B = 16 389 > 2 x 2048 x 4: k_head_fwd at its 2048-workgroup cap, five waves take a second trip in which no second '
      'row exists.  no tag: the cap', HEAD_FWD_CAP_ROWS + 5, 64, 1)
_head('head_no_dx', 'dx = NULL: head_ok of the backward does not ask for its alignment; dkernel and dbias only', 9, 64, 1, want=('dkernel', 'dbias'),
      dx='none')
_head('head_dx_only', 'dkernel = dbias = NULL: k_head_dx alone, nothing touches the workspace', 131, 256, 1, want=('dx',),
      dkernel='none', dbias='none')
row('head_d60_gemm', 'D = 60 < 64: below head_ok, every product on the GEMM', 9, 60, 1)
row('head_d66_gemm', 'D = 66: D % 4 != 0, every product on the GEMM', 9, 66, 1)
row('head_d4100_gemm', 'D = 4100 > 4096: above head_ok, every product on the GEMM', 9, 4100, 1)
row('head_x_off1', 'head shape with x one float past a 16-byte boundary: head_ok fails in both calls, the GEMM reads the unaligned rows', 131, 64, 1,
    x_off=1)
row('head_dx_off1', 'head shape with dx one float past a 16-byte boundary: the forward takes k_head_fwd<1>, the backward fails head_ok and runs '
    'dkernel and dx as GEMMs (unaligned C), dbias as a column sum', 131, 64, 1, dx_off=1, y='head_fwd<1>')
row('u1_n2_not_head', 'U = 1 with N = 2: not the head (N = 1 only); batched GEMMs, one column sum per expert (U < 64)', 131, 64, 1, N=2, xb=1,
    dx='gemm_batched')
# ---- narrow kernels (k_narrow_dense as forward and as dx) -----------------------------------------------------------------------------------------
_BN = NARROW_MIN_B + 37            # a ragged last tile of ND_ROWS = 64 (37 rows) and of XTY_ROWS = 32
row('gemm_b4095', 'B = 4095: one row below narrow_ok and xty_ok, every product on the GEMM', 4095, 64, 32)
row('narrow_4x4', '(4, 4): k_narrow_dense<1> both ways; D U = 16: dkernel on the GEMM', _BN, 4, 4, y='narrow', dx='narrow')
row('narrow_64x32', '(64, 32): k_narrow_dense<8> forward, <16> as dx; k_small_xty<8> with fused bias sums', _BN, 64, 32, y='narrow', dx='narrow',
    dkernel='xty<8>', dbias='xty_fused')
row('narrow_32x64', '(32, 64): k_narrow_dense<16> forward, <8> as dx; k_small_xty<8>', _BN, 32, 64, y='narrow', dx='narrow', dkernel='xty<8>',
    dbias='xty_fused')
row('narrow_128x32', '(128, 32): D at the edge, D U = 4096 at the edge: k_narrow_dense<8> / <32>; k_small_xty<16>', _BN, 128, 32, y='narrow',
    dx='narrow', dkernel='xty<16>', dbias='xty_fused')
row('narrow_32x128', '(32, 128): U at the edge: k_narrow_dense<32> / <8>; k_small_xty<16>', _BN, 32, 128, y='narrow', dx='narrow', dkernel='xty<16>',
    dbias='xty_fused')
row('narrow_12x20', '(12, 20): narrow (k_narrow_dense<5> / <3>), D U = 240 is no multiple of 256: dkernel on the GEMM', _BN, 12, 20, y='narrow',
    dx='narrow')
row('narrow_24x32', '(24, 32): narrow; D U / 256 = 3 is no k_small_xty instance: dkernel on the GEMM', _BN, 24, 32, y='narrow', dx='narrow')
row('gemm_132x4', '(132, 4): D > 128, neither narrow nor register-tile: every product on the GEMM', _BN, 132, 4)
row('narrow_stride_b131141', 'B = 131 141 > 2048 x 64 rows: k_narrow_dense at its workgroup cap, two workgroups walk a second tile, the last one '
    'ragged (5 rows).  no tag: the cap', NARROW_CAP_ROWS + ND_ROWS + 5, 4, 4, y='narrow', dx='narrow')
row('n2_narrow_shape', 'a narrow and register-tile shape with N = 2: both predicates want N = 1, batched GEMMs', _BN, 16, 16, N=2, xb=1,
    dx='gemm_batched')
# ---- k_small_xty ------------------------------------------------------------------------------------------------------------------------------
row('xty1_16x16', '(16, 16): k_small_xty<1>, narrow both ways.  no tag: the instance', _BN, 16, 16, y='narrow', dx='narrow', dkernel='xty<1>',
    dbias='xty_fused')
row('xty1_2x128', '(2, 128): k_small_xty<1> (only threads 0..127 own bias sums), D % 4 != 0: y and dx on the GEMM', _BN, 2, 128, dkernel='xty<1>',
    dbias='xty_fused')
row('xty1_128x2', '(128, 2): k_small_xty<1> (threads 0, 1 own the bias sums), U % 4 != 0: y and dx on the GEMM', _BN, 128, 2, dkernel='xty<1>',
    dbias='xty_fused')
row('xty2_16x32_no_dbias', '(16, 32): k_small_xty<2> without dbias (part_b = NULL)', _BN, 16, 32, want=('dx', 'dkernel'), y='narrow', dx='narrow',
    dkernel='xty<2>', dbias='none')
row('xty4_32x32_no_dx', '(32, 32): k_small_xty<4> (float4 reads of dZ); dx = NULL', _BN, 32, 32, want=('dkernel', 'dbias'), y='narrow', dx='none',
    dkernel='xty<4>', dbias='xty_fused')
row('xty_no_dkernel', '(64, 32) with dkernel = NULL: no register-tile pass, dbias from the column sum of dZ; dx narrow', _BN, 64, 32,
    want=('dx', 'dbias'), y='narrow', dx='narrow', dkernel='none', dbias='colsum')
row('xty_cap_b131207', 'B = 131 207 > 1024 x 128 rows: k_small_xty at its 1024-workgroup cap (129 rows per workgroup, the last one short).  '
    'no tag: the cap', XTY_CAP_ROWS + 128 + 7, 16, 16, y='narrow', dx='narrow', dkernel='xty<1>', dbias='xty_fused')
# ---- general route -------------------------------------------------------------------------------------------------------------------------------
row('gen_batched_n3_u63', 'N = 3, batched x, U = 63: batched GEMMs; bias sums one per expert (U < 64).  no tag: which bias sum', 131, 40, 63, N=3,
    xb=1, dx='gemm_batched')
row('gen_bcast_n3_u64', 'N = 3, broadcast x, U = 64: dx = three products accumulated in order; rn_colsum_batched.  no tag: which bias sum', 131, 40,
    64, N=3, dbias='colsum_batched')
row('gen_batched_n2_u200', 'N = 2, batched x, U = 200 (a ragged column tile), B = 300: batched bias sums', 300, 96, 200, N=2, xb=1,
    dx='gemm_batched', dbias='colsum_batched')
row('gen_b1', 'B = 1: one row through every GEMM and column sum', 1, 7, 5, N=2)
row('gen_bcast_n1', 'N = 1 with broadcast x below every fast route: one product for dx', 131, 40, 24)
# ---- empty batch -----------------------------------------------------------------------------------------------------------------------------------
row('empty', 'B = 0: RECNOW_OK, no launch, dkernel and dbias zeroed', 0, 8, 4, N=2, y='none', dkernel='zero', dbias='zero', dx='none')

KERNEL_INSTANCES = {
    'y': ('head_fwd<1>', 'head_fwd<4>', 'head_fwd<16>', 'narrow', 'gemm', 'none'),
    'dkernel': ('head_dw', 'xty<1>', 'xty<2>', 'xty<4>', 'xty<8>', 'xty<16>', 'gemm', 'none', 'zero'),
    'dbias': ('colsum', 'colsum_batched', 'xty_fused', 'none', 'zero'),
    'dx': ('head_dx', 'narrow', 'gemm_batched', 'gemm_bcast', 'none'),
}


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
# integer data: integers times powers of two; every product and partial sum is then a multiple of the grid below
X_SCALE, K_SCALE, B_SCALE, DY_SCALE = 0.5, 0.25, 0.125, 0.5


def seed_of(name):
    import zlib
    return zlib.crc32(name.encode())


def shapes(r):
    B, D, U, N = r['B'], r['D'], r['U'], r['N']
    return dict(x=(N, B, D) if r['x_batched'] else (B, D), kernel=(N, D, U), bias=(N, U), dy=(N, B, U))


def integer_inputs(r):
    """x in {-2..2} / 2, kernel in {-1, 0, 1} / 4, bias in {-4..4} / 8, dy in {-2..2} / 2 (float64 arrays)"""
    import numpy as np
    rng = np.random.default_rng(seed_of(r['name']))
    s = shapes(r)
    return dict(x=rng.integers(-2, 3, s['x']) * X_SCALE, kernel=rng.integers(-1, 2, s['kernel']) * K_SCALE,
                bias=rng.integers(-4, 5, s['bias']) * B_SCALE, dy=rng.integers(-2, 3, s['dy']) * DY_SCALE)


def random_inputs(r):
    """Rows of x scaled by 2^-k, columns of kernel likewise (k cycling through 0..8).  The pre-activation is bias (0.25 <= |bias| <= 0.5) plus a
    product of standard deviation <= 0.04: no entry of y is a cancelled sum, so `1e-5 x the row's max |ref|` is a bound fp32 can meet even where
    the row has ONE entry (the scoring head), and TANH / SIGMOID stay away from saturation (the backward reads act' from the fp32 y).  With fewer
    than four entries per row of dx (D < 4) kernel and dy are positive, for the same reason."""
    import numpy as np
    rng = np.random.default_rng(seed_of(r['name']) + 1)
    B, D, U, N = r['B'], r['D'], r['U'], r['N']
    s = shapes(r)
    x = rng.uniform(-1, 1, s['x']) * np.exp2(-(np.arange(B) % 9).astype(np.float64))[:, None]
    k = rng.standard_normal(s['kernel']) * (0.07 / np.sqrt(D)) * np.exp2(-(np.arange(U) % 9).astype(np.float64))[None, None, :]
    bias = rng.uniform(0.25, 0.5, s['bias']) * rng.choice([-1.0, 1.0], s['bias'])
    dy = rng.uniform(-1, 1, s['dy'])
    if D < 4:
        k, dy = np.abs(k), np.abs(dy)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    return dict(x=f32(x), kernel=f32(k), bias=f32(bias), dy=f32(dy))


def _act(z, act):
    import numpy as np
    return z if act == LINEAR else np.maximum(z, 0.0) if act == RELU else np.tanh(z) if act == TANH else 1.0 / (1.0 + np.exp(-z))


def _act_grad(y, act):
    import numpy as np
    return np.ones_like(y) if act == LINEAR else (y > 0).astype(np.float64) if act == RELU else 1.0 - y * y if act == TANH else y * (1.0 - y)


def reference(r, inp, act):
    """fp64 MultiDense forward and backward of the float64 inputs.  Returns (out, mag): out = y, dx, dkernel, dbias; mag = for each of them the
    sum of |terms| of every entry (the scale of a sum that may cancel, and the bound of every partial sum in any order)."""
    import numpy as np
    x, k, bias, dy = inp['x'], inp['kernel'], inp['bias'], inp['dy']
    xb = x if r['x_batched'] else np.broadcast_to(x, (r['N'],) + x.shape)
    z = np.matmul(xb, k) + bias[:, None, :]
    y = _act(z, act)
    dz = dy * _act_grad(y, act)
    dxn = np.matmul(dz, k.transpose(0, 2, 1))
    out = dict(y=y, dkernel=np.matmul(xb.transpose(0, 2, 1), dz), dbias=dz.sum(1), dx=dxn if r['x_batched'] else dxn.sum(0))
    mdx = np.matmul(np.abs(dz), np.abs(k).transpose(0, 2, 1))
    mag = dict(y=np.matmul(np.abs(xb), np.abs(k)) + np.abs(bias)[:, None, :], dkernel=np.matmul(np.abs(xb).transpose(0, 2, 1), np.abs(dz)),
               dbias=np.abs(dz).sum(1), dx=mdx if r['x_batched'] else mdx.sum(0))
    return out, mag


GRID = dict(y=X_SCALE * K_SCALE, dkernel=X_SCALE * DY_SCALE, dbias=DY_SCALE, dx=DY_SCALE * K_SCALE)      # (bias is a multiple of x * kernel's grid)

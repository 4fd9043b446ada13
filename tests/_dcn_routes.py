"""The route table of DCNLayer's C entry points (csrc/dcn.hip recnow_dcn_fwd / recnow_dcn_bwd, recnow_dcn_step_fwd / _bwd): one row per distinct path,
with the call that reaches it, and a Python mirror of the route choice (csrc/dcn.hip dcn_route_fwd / dcn_route_bwd, queried through
recnow_dcn_route).  Used by tests/test_dcn_routes_gpu.py (every row on the GPU against fp64, and the linear and relu rows bit for bit on census data) and
tests/test_dcn_census_cpu.py (mirror == query; the census of every linear and relu row is exact and has teeth).

How a call picks its kernels (mis: the tensors that start off a 16-byte boundary):
  pick(D, aligned)    aligned = D % 4 == 0 and the three streamed tensors aligned (forward x, y, kernels; backward x, dy, dx):
                      D <= 256: (64, 4, 1); <= 1024: (64, 4, 4); <= 4096: (256, 4, 4); else none.  Not aligned: D <= 256: (256, 1, 1); <= 1024: (256, 1, 4);
                      else none.  (tpr, vec, nv): threads per row, floats per access, register images per thread
  forward             no pick, or biases misaligned under a vec-4 pick: k_dcn_fwd_general.  Else FAST (k_dcn_fwd_fast<NV, L, ACT, CS>) when tpr = 64,
                      vec = 4, D = 256 nv, B % 4 == 0, L <= 4 and 8 L D <= 48 KiB; else k_dcn_fwd<tpr, vec, nv>
  backward            L > 4, no pick, or kernels / biases misaligned under a vec-4 pick: the general rows + columns kernels.  Without csave the pick
                      maps (64, 4, 4) to (256, 4, 1) and k_dcn_bwd<..> recomputes the forward per row.  With csave: (64, 4, 4) with L > 3 becomes
                      (128, 4, 2); FAST (k_dcn_bwd_fast<TPR, NV, L, ACT>) when vec = 4, D = 4 tpr nv, B % (256 / tpr) == 0, tpr in {64, 128}, the
                      combine rows + 8 L D <= 48 KiB and the instantiation exists ((64, 1, 1..4), (64, 4, 1..3), (128, 2, 1..4)); else
                      k_dcn_bwd_saved_wl<..> when the combine rows + 8 L D <= 48 KiB, else k_dcn_bwd_saved<..>
  instantiations that no call reaches
                      k_dcn_bwd_fast<128, 2, L> for L = 1, 2, 3 (tpr = 128 is chosen only for L > 3); the (128, 4, 2) instantiations of k_dcn_fwd,
                      k_dcn_bwd and k_dcn_bwd_saved (the forward and the recompute backward never pick tpr = 128; at D <= 1024, L = 4 the LDS need is
                      40 KiB, so _wl always takes it); k_dcn_bwd<64, 4, 4> (remapped to (256, 4, 1)); k_dcn_bwd_saved<64, 4, 1>, <64, 4, 4>, <256, 1, 1>
                      and <256, 1, 4> (D <= 1024 and L <= 4 fit 48 KiB); k_dcn_bwd_saved<256, 4, 1>, k_dcn_bwd_saved_wl<256, 4, 1> and k_dcn_fwd<256, 4, 1>
                      ((256, 4, 1) only comes from the recompute remap)

Row fields: name, B, D, L, act (RECNOW_ACT_* code), bias, csave (the forward writes it and the backward reads it; False: NULL in both), lead
(tensor -> floats past a 16-byte boundary, as _guard.Buf(lead=..); tensors: x, y, dy, dx, kernels, biases), fwd / bwd (the expected route codes),
why."""
LINEAR, RELU, TANH, SIGMOID = 0, 1, 2, 3
MIS_X, MIS_Y, MIS_DX, MIS_K, MIS_B = 1, 2, 4, 8, 16
F_GENERAL, F_TEMPLATED, F_FAST = 1, 2, 3
B_GENERAL, B_RECOMPUTE, B_SAVED, B_SAVED_WL, B_FAST = 1, 2, 3, 4, 5
MAX_L = 4
LDS = 48 * 1024


def code(family, cfg=(0, 0, 0)):
    return family * 100000 + cfg[0] * 100 + cfg[1] * 10 + cfg[2]


def pick(D, ptrs_aligned):
    if ptrs_aligned and D % 4 == 0:
        return (64, 4, 1) if D <= 256 else (64, 4, 4) if D <= 1024 else (256, 4, 4) if D <= 4096 else None
    return (256, 1, 1) if D <= 256 else (256, 1, 4) if D <= 1024 else None


def route_fwd(B, D, L, mis=0):
    cfg = pick(D, not mis & (MIS_X | MIS_Y | MIS_K))
    if cfg is None or (mis & MIS_B and cfg[1] == 4):
        return code(F_GENERAL)
    fast = cfg[:2] == (64, 4) and D == 256 * cfg[2] and B % 4 == 0 and L <= MAX_L and 8 * L * D <= LDS
    return code(F_FAST if fast else F_TEMPLATED, cfg)


def fast_bwd_built(cfg, L):
    return 1 <= L <= {(64, 1): 4, (128, 2): 4, (64, 4): 3}.get((cfg[0], cfg[2]), 0)


def route_bwd(B, D, L, csave, mis=0):
    cfg = pick(D, not mis & (MIS_X | MIS_Y | MIS_DX))
    if not csave and cfg == (64, 4, 4):
        cfg = (256, 4, 1)
    if L > MAX_L or cfg is None or (cfg[1] == 4 and mis & (MIS_K | MIS_B)):
        return code(B_GENERAL)
    if csave and cfg == (64, 4, 4) and L > 3:
        cfg = (128, 4, 2)
    tpr, vec, nv = cfg
    lds = (256 // tpr * D * 4 if tpr < 256 else 0) + 8 * L * D
    if not csave:
        return code(B_RECOMPUTE, cfg)
    if vec == 4 and D == tpr * 4 * nv and B % (256 // tpr) == 0 and tpr in (64, 128) and lds <= LDS and fast_bwd_built(cfg, L):
        return code(B_FAST, cfg)
    return code(B_SAVED_WL if lds <= LDS else B_SAVED, cfg)


def route(which, B, D, L, csave, mis):
    """the mirror of recnow_dcn_route"""
    if B == 0:
        return 0
    return route_bwd(B, D, L, csave, mis) if which else route_fwd(B, D, L, mis)


def masks(r):
    """(forward, backward) align_mask of a row"""
    ld = r['lead']
    b = MIS_B if (r['bias'] and ld.get('biases', 0) % 4) else 0
    k = MIS_K if ld.get('kernels', 0) % 4 else 0
    x = MIS_X if ld.get('x', 0) % 4 else 0
    return (x | (MIS_Y if ld.get('y', 0) % 4 else 0) | k | b,
            x | (MIS_Y if ld.get('dy', 0) % 4 else 0) | (MIS_DX if ld.get('dx', 0) % 4 else 0) | k | b)


ROUTES = []
ACT_NAME = {LINEAR: 'lin', RELU: 'relu', TANH: 'tanh', SIGMOID: 'sig'}


def row(name, why, fwd, bwd, B, D, L, act=LINEAR, bias=True, csave=True, lead=None):
    assert name not in {r['name'] for r in ROUTES}, name
    ROUTES.append(dict(name=name, B=B, D=D, L=L, act=act, bias=bias, csave=csave, lead=dict(lead or {}), fwd=code(*fwd), bwd=code(*bwd), why=why))


C641, C644, C1282, C2561, C2564, S2561, S2564 = (64, 4, 1), (64, 4, 4), (128, 4, 2), (256, 4, 1), (256, 4, 4), (256, 1, 1), (256, 1, 4)


def _fast_bwd_cfg(D, L):
    return C641 if D == 256 else C644 if L <= 3 else C1282


# ---- fast forward and fast backward: B = 4 (one workgroup: the next-row request clamps on the first pass) ------------------------------------------------
for _D in (256, 1024):
    for _L in (1, 2, 3, 4):
        _cf = C641 if _D == 256 else C644
        for _a in (LINEAR, TANH):
            row('fast_d%d_l%d_%s_b4' % (_D, _L, ACT_NAME[_a]), 'k_dcn_fwd_fast<%d, %d, %s, true> and k_dcn_bwd_fast<%d, %d, %d>, one workgroup' % (
                (_cf[2], _L, 'LINEAR' if _a == LINEAR else '-1') + (_fast_bwd_cfg(_D, _L)[0], _fast_bwd_cfg(_D, _L)[2], _L)),
                (F_FAST, _cf), (B_FAST, _fast_bwd_cfg(_D, _L)), 4, _D, _L, act=_a)
            row('fast_d%d_l%d_%s_b4_nocsave' % (_D, _L, ACT_NAME[_a]), 'k_dcn_fwd_fast<.., CS = false>; the backward recomputes: k_dcn_bwd<%s>' % (
                '64, 4, 1' if _D == 256 else '256, 4, 1 (the dcn_pick_bwd remap of 1024-wide rows)'),
                (F_FAST, _cf), (B_RECOMPUTE, C641 if _D == 256 else C2561), 4, _D, _L, act=_a, csave=False)
        row('fast_d%d_l%d_sig_b4' % (_D, _L), 'the runtime-activation instantiation with sigmoid', (F_FAST, _cf), (B_FAST, _fast_bwd_cfg(_D, _L)), 4, _D, _L,
            act=SIGMOID)
# B = 8196 = 4 * 2049: dcn_grid caps the grid at 2048, workgroup 0 makes two passes and the others one
for _D in (256, 1024):
    for _L in (1, 2, 3, 4):
        _cf = C641 if _D == 256 else C644
        for _a in (LINEAR, TANH, SIGMOID):
            row('fast_d%d_l%d_%s_b8196' % (_D, _L, ACT_NAME[_a]), '2049 row groups on at most 2048 workgroups: grid-stride loop, the next-row request of the '
                'last pass clamps to the own row; the backward grid is capped at one resident wave of workgroups, so its workgroups make several passes',
                (F_FAST, _cf), (B_FAST, _fast_bwd_cfg(_D, _L)), 8196, _D, _L, act=_a)
row('fast_d256_l2_lin_b8196_nocsave', 'CS = false on the two-pass grid; k_dcn_bwd<64, 4, 1> over 2048 workgroups', (F_FAST, C641), (B_RECOMPUTE, C641), 8196, 256, 2,
    csave=False)
row('fast_d1024_l3_tanh_b8196_nocsave', 'CS = false on the two-pass grid; k_dcn_bwd<256, 4, 1> strides 8196 rows over 2048 workgroups', (F_FAST, C644),
    (B_RECOMPUTE, C2561), 8196, 1024, 3, act=TANH, csave=False)
for _a in (LINEAR, TANH, SIGMOID):
    row('fast128_b8198_%s' % ACT_NAME[_a], 'B = 8198 is even and no multiple of 4: the forward is k_dcn_fwd<64, 4, 4>, the backward k_dcn_bwd_fast<128, 2, 4> '
        '(two waves per row combined through LDS, two rows per workgroup)', (F_TEMPLATED, C644), (B_FAST, C1282), 8198, 1024, 4, act=_a)

# ---- fall-backs next to the fast routes --------------------------------------------------------------------------------------------------------
for _B in (1001, 6):
    row('fallback_d256_b%d' % _B, 'B %% 4 != 0 fails both fast guards: k_dcn_fwd<64, 4, 1> and k_dcn_bwd_saved_wl<64, 4, 1> on full lanes', (F_TEMPLATED, C641),
        (B_SAVED_WL, C641), _B, 256, 3, act=TANH)
    row('fallback_d1024_l3_b%d' % _B, 'B %% 4 != 0: k_dcn_fwd<64, 4, 4> and k_dcn_bwd_saved_wl<64, 4, 4> on full lanes', (F_TEMPLATED, C644), (B_SAVED_WL, C644),
        _B, 1024, 3)
row('fallback_d1024_l4_b1001', 'odd B at L = 4: the backward falls to k_dcn_bwd_saved_wl<128, 4, 2>', (F_TEMPLATED, C644), (B_SAVED_WL, C1282), 1001, 1024, 4,
    act=SIGMOID)
row('fallback_d1024_l4_b6', 'B = 6 fails the forward guard (B % 4) and passes the backward one (B % 2): the backward stays on k_dcn_bwd_fast<128, 2, 4>',
    (F_TEMPLATED, C644), (B_FAST, C1282), 6, 1024, 4, act=TANH)
row('l5_d256', 'L = 5 > DCN_MAX_L: the forward is the layer loop of k_dcn_fwd<64, 4, 1> without register-resident weights, the backward general',
    (F_TEMPLATED, C641), (B_GENERAL,), 8, 256, 5, act=TANH)

# ---- the seven (tpr, vec, nv) configurations of the templated kernels, with a D that fills the lanes and one that does not -------------------------------
_T = [(4, 37, 2, TANH), (252, 37, 3, LINEAR), (260, 37, 3, RELU), (512, 37, 4, TANH), (1020, 21, 2, LINEAR), (1028, 21, 3, SIGMOID), (4096, 5, 1, LINEAR)]
for _D, _B, _L, _a in _T:
    _cf = pick(_D, True)
    _cs = C1282 if (_cf == C644 and _L > 3) else _cf
    row('templ_d%d_l%d' % (_D, _L), 'aligned D = %d: k_dcn_fwd<%r>, k_dcn_bwd_saved_wl<%r>' % (_D, _cf, _cs), (F_TEMPLATED, _cf), (B_SAVED_WL, _cs), _B, _D, _L,
        act=_a)
    _cr = C2561 if _cf == C644 else _cf
    row('templ_d%d_l%d_nocsave' % (_D, _L), 'aligned D = %d without csave: k_dcn_bwd<%r>' % (_D, _cr), (F_TEMPLATED, _cf), (B_RECOMPUTE, _cr), _B, _D, _L,
        act=_a, csave=False)
for _D, _B, _L, _a in [(3, 37, 4, LINEAR), (255, 37, 2, TANH), (257, 37, 3, LINEAR), (1023, 21, 4, RELU)]:
    _cf = pick(_D, False)
    row('templ_d%d_l%d' % (_D, _L), 'D %% 4 != 0: the scalar configuration %r in k_dcn_fwd and k_dcn_bwd_saved_wl' % (_cf,), (F_TEMPLATED, _cf), (B_SAVED_WL, _cf),
        _B, _D, _L, act=_a)
    row('templ_d%d_l%d_nocsave' % (_D, _L), 'D %% 4 != 0 without csave: k_dcn_bwd<%r>' % (_cf,), (F_TEMPLATED, _cf), (B_RECOMPUTE, _cf), _B, _D, _L, act=_a,
        csave=False)
row('saved_wl_d2048_l2', '4 L D 2 = 32 KiB <= 48 KiB: k_dcn_bwd_saved_wl<256, 4, 4> (weights staged in LDS)', (F_TEMPLATED, C2564), (B_SAVED_WL, C2564), 9, 2048, 2,
    act=TANH)
row('saved_d2048_l4', '64 KiB > 48 KiB: k_dcn_bwd_saved<256, 4, 4> (weights from global memory)', (F_TEMPLATED, C2564), (B_SAVED, C2564), 9, 2048, 4)
row('saved_d4096_l3', 'the widest register image, L = 3: 96 KiB, k_dcn_bwd_saved<256, 4, 4>', (F_TEMPLATED, C2564), (B_SAVED, C2564), 5, 4096, 3, act=SIGMOID)
row('templ_two_pass_rpb1', 'B = 2051 rows on 2048 one-row workgroups: the grid-stride loop and next-row request of the (256, 4, 4) kernels', (F_TEMPLATED, C2564),
    (B_SAVED_WL, C2564), 2051, 1028, 2)
row('templ_two_pass_rpb4', 'B = 8195 rows on 2048 four-row workgroups: second pass with a ragged last workgroup, (64, 4, 1) with idle lanes',
    (F_TEMPLATED, C641), (B_SAVED_WL, C641), 8195, 252, 3)
row('templ_two_pass_rpb4_nocsave', 'the same rows through k_dcn_bwd<64, 4, 1> (recompute)', (F_TEMPLATED, C641), (B_RECOMPUTE, C641), 8195, 252, 2, act=TANH,
    csave=False)

# ---- misalignment: one tensor one float off a 16-byte boundary, at sizes the fast kernels take -----------------------------------------------------------
for _D in (256, 1024):
    _cf, _sc = (C641, S2561) if _D == 256 else (C644, S2564)
    row('mis_x_d%d' % _D, 'x off: the scalar configuration in both directions', (F_TEMPLATED, _sc), (B_SAVED_WL, _sc), 8, _D, 3, lead={'x': 1})
    row('mis_y_d%d' % _D, 'y off: scalar forward; the backward does not see y', (F_TEMPLATED, _sc), (B_FAST, _cf), 8, _D, 3, act=TANH, lead={'y': 1})
    row('mis_dy_d%d' % _D, 'dy off: the forward stays fast, scalar backward', (F_FAST, _cf), (B_SAVED_WL, _sc), 8, _D, 3, lead={'dy': 1})
    row('mis_dx_d%d' % _D, 'dx off: the forward stays fast, scalar backward', (F_FAST, _cf), (B_SAVED_WL, _sc), 8, _D, 3, act=TANH, lead={'dx': 3})
    row('mis_kernels_d%d' % _D, 'kernels off: scalar forward (kernels is one of its three streamed tensors); vec-4 backward pick with misaligned weights: general',
        (F_TEMPLATED, _sc), (B_GENERAL,), 8, _D, 3, lead={'kernels': 1})
    row('mis_biases_d%d' % _D, 'biases off under a vec-4 pick: general in both directions', (F_GENERAL,), (B_GENERAL,), 8, _D, 3, act=TANH, lead={'biases': 1})
    row('mis_biases_null_d%d' % _D, 'no bias: a NULL biases pointer is aligned, the fast kernels fill zeros', (F_FAST, _cf), (B_FAST, _cf), 8, _D, 2, bias=False,
        lead={'biases': 1})
    row('mis_x_kernels_nocsave_d%d' % _D, 'x and kernels off, no csave: scalar pick, where misaligned weights do not matter: k_dcn_bwd scalar', (F_TEMPLATED, _sc),
        (B_RECOMPUTE, _sc), 8, _D, 2, csave=False, lead={'x': 2, 'kernels': 1})

# ---- general path -----------------------------------------------------------------------------------------------------------------------------
for _cs in (True, False):
    _s = '' if _cs else '_nocsave'
    row('general_d4100' + _s, 'D > 4096: k_dcn_fwd_general, rows + columns kernels' + ('' if _cs else '; the backward makes its own scalars'), (F_GENERAL,),
        (B_GENERAL,), 33, 4100, 2, act=TANH, csave=_cs)
    row('general_d1025' + _s, 'D = 1025 unaligned and > 1024; B = 300: two slabs of k_dcn_bwd_cols_general', (F_GENERAL,), (B_GENERAL,), 300, 1025, 3, csave=_cs)
    row('general_l6' + _s, 'L = 6 at D = 256: templated forward loop, general backward', (F_TEMPLATED, C641), (B_GENERAL,), 10, 256, 6, act=SIGMOID, csave=_cs)
row('general_d1025_relu', 'relu on the general path (pre-activations kept off zero)', (F_GENERAL,), (B_GENERAL,), 19, 1025, 2, act=RELU)

# ---- no bias ----------------------------------------------------------------------------------------------------------------------------------
row('nobias_fast', 'biases = dbiases = NULL on the fast kernels (LDS bias rows are zeros)', (F_FAST, C644), (B_FAST, C644), 8, 1024, 3, act=TANH, bias=False)
row('nobias_templ', 'biases = dbiases = NULL on k_dcn_fwd<64, 4, 4> / k_dcn_bwd_saved_wl<64, 4, 4>', (F_TEMPLATED, C644), (B_SAVED_WL, C644), 9, 260, 2, bias=False)
row('nobias_templ_nocsave', 'biases = dbiases = NULL on k_dcn_bwd<256, 4, 1>', (F_TEMPLATED, C644), (B_RECOMPUTE, C2561), 9, 260, 2, act=SIGMOID, bias=False,
    csave=False)
row('nobias_saved', 'biases = NULL on k_dcn_bwd_saved<256, 4, 4> (reads weights from global memory)', (F_TEMPLATED, C2564), (B_SAVED, C2564), 5, 2048, 4, act=TANH,
    bias=False)
row('nobias_general', 'biases = dbiases = NULL on the general path', (F_GENERAL,), (B_GENERAL,), 19, 1025, 2, act=TANH, bias=False)

# ---- the step route: one cross layer with its own layer input (recnow_dcn_step_fwd / _bwd; one kernel family, any D, any alignment) ------------------------
STEPS = [dict(name='step_d%d_%s%s' % (D, ACT_NAME[a], '' if bias else '_nobias'), B=B, D=D, act=a, bias=bias)
         for D, B in ((96, 300), (1024, 300), (5000, 70)) for a in (LINEAR, TANH) for bias in ((True, False) if D == 96 else (True,))]

BY_NAME = {r['name']: r for r in ROUTES}


def sweep_D():
    """every D of 1 .. 4200 within 1 of a boundary of pick() or of the LDS rules, and a coarse grid between"""
    ds = set(range(1, 10)) | set(range(1, 4201, 97))
    for b in (256, 512, 768, 1024, 1536, 2048, 3072, 4096, 4200):
        ds |= {d for d in range(b - 5, b + 6) if 1 <= d <= 4200}
    return sorted(ds)

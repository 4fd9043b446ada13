"""CPU: the route table of DCN-v1 (tests/_dcn_routes.py) and its census (tests/_dcn_census.py) are what tests/test_dcn_routes_gpu.py takes them for.
  * the Python mirror of the route choice equals recnow_dcn_route (a host function of csrc/dcn.hip: no device needed) on every row and over a sweep;
  * the table reaches every kernel instantiation a call can reach;
  * the closed form the scales come from equals oracle/dense_ref.dcn_layer under fp64 autograd;
  * census: on every linear and relu row every sum any kernel forms keeps sum |terms| < 2^24 on the first ladder entry, and an fp32 restatement in
    the kernels' factorisation returns the fp64 values to the bit; with each planted mistake it does not;
  * random data: the fp32 restatement stays under half the 1e-5 bound on every row (the data, not the bound, was chosen for that)."""
import numpy as np
import pytest
import torch

import _dcn_census as C
import _dcn_routes as T
import dense_ref as R


def _lib():
    from rec_now_amd import _lib
    return _lib.load()


def test_table_matches_mirror_and_query():
    lib = _lib()
    for r in T.ROUTES:
        mf, mb = T.masks(r)
        for which, mask, want in ((0, mf, r['fwd']), (1, mb, r['bwd'])):
            assert T.route(which, r['B'], r['D'], r['L'], r['csave'], mask) == want, (r['name'], which)
            assert lib.recnow_dcn_route(which, r['B'], r['D'], r['L'], int(r['csave']), mask) == want, (r['name'], which)


def test_mirror_matches_query_over_sweep():
    lib = _lib()
    ds = T.sweep_D()
    assert {1, 255, 256, 257, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 4200} <= set(ds)
    n = 0
    for D in ds:
        for L in range(1, 9):
            for B in (1, 2, 3, 4, 6, 8):
                for mask in range(32):
                    for cs in (0, 1):
                        for which in (0, 1):
                            got = lib.recnow_dcn_route(which, B, D, L, cs, mask)
                            assert got == T.route(which, B, D, L, cs, mask), (which, B, D, L, cs, mask, got)
                            n += 1
    assert n == len(ds) * 8 * 6 * 32 * 2 * 2
    assert lib.recnow_dcn_route(0, 0, 256, 3, 1, 0) == 0 and lib.recnow_dcn_route(1, 0, 256, 3, 1, 0) == 0
    for bad in ((2, 8, 256, 3, 1, 0), (0, -1, 256, 3, 1, 0), (0, 8, 0, 3, 1, 0), (1, 8, 256, 0, 1, 0), (1, 8, 256, 3, 1, 32), (0, 8, 256, 3, 0, -1)):
        assert lib.recnow_dcn_route(*bad) == -1, bad


def test_table_reaches_every_reachable_instantiation():
    """what the drivers can launch, enumerated from the mirror over the sweep (every B residue, every mask): each (family, cfg) -- and for the fast
    kernels each (cfg, L, compile-time or runtime activation, csave) -- has a row"""
    reach = set()
    for D in T.sweep_D():
        for L in range(1, 9):
            for B in (1, 2, 3, 4, 6, 8):
                for mask in (0, 1, 2, 4, 8, 16):
                    for cs in (0, 1):
                        f, b = T.route(0, B, D, L, cs, mask), T.route(1, B, D, L, cs, mask)
                        reach.add(('fwd', f, L if f // 100000 == T.F_FAST else 0))
                        reach.add(('bwd', b, L if b // 100000 == T.B_FAST else 0))
    have = set()
    for r in T.ROUTES:
        have.add(('fwd', r['fwd'], r['L'] if r['fwd'] // 100000 == T.F_FAST else 0))
        have.add(('bwd', r['bwd'], r['L'] if r['bwd'] // 100000 == T.B_FAST else 0))
    assert reach == have, (sorted(reach - have), sorted(have - reach))
    fast_f = {(r['fwd'], r['L'], r['act'] == T.LINEAR, r['csave']) for r in T.ROUTES if r['fwd'] // 100000 == T.F_FAST}
    assert fast_f == {(T.code(T.F_FAST, cfg), L, lin, cs) for cfg in (T.C641, T.C644) for L in (1, 2, 3, 4) for lin in (True, False) for cs in (True, False)}
    fast_b = {(r['bwd'], r['L'], r['act'] == T.LINEAR) for r in T.ROUTES if r['bwd'] // 100000 == T.B_FAST}
    want = {(T.C641, L) for L in (1, 2, 3, 4)} | {(T.C644, L) for L in (1, 2, 3)} | {(T.C1282, 4)}
    assert fast_b == {(T.code(T.B_FAST, cfg), L, lin) for cfg, L in want for lin in (True, False)}
    # both passes counts of the grid-stride loops, and every activation on the fast backward
    for cfg, L in want:
        rows = [r for r in T.ROUTES if r['bwd'] == T.code(T.B_FAST, cfg) and r['L'] == L]
        for small in (True, False):                      # one workgroup (B <= 8), and B >= 8196: several passes of the grid-stride loop
            acts = {r['act'] for r in rows if (r['B'] <= 8) == small and (small or r['B'] >= 8196)}
            assert acts >= {T.LINEAR, T.TANH, T.SIGMOID}, (cfg, L, small)
    # the fast forward: every (nv, L), linear and tanh, with csave, at B = 4 and at B = 8196
    for cfg in (T.C641, T.C644):
        for L in (1, 2, 3, 4):
            for Bv in (4, 8196):
                acts = {r['act'] for r in T.ROUTES if r['fwd'] == T.code(T.F_FAST, cfg) and r['L'] == L and r['B'] == Bv and r['csave']}
                assert acts >= {T.LINEAR, T.TANH}, (cfg, L, Bv)
    assert all(r['B'] <= 8200 and r['B'] * r['D'] <= 8.4e6 for r in T.ROUTES)


@pytest.mark.parametrize('act', [C.LINEAR, C.RELU, C.TANH, C.SIGMOID])
@pytest.mark.parametrize('bias', [True, False])
def test_closed_form_is_the_autograd_oracle(act, bias):
    r = dict(name='closed form %d %d' % (act, bias), B=23, D=37, L=4, act=act, bias=bias)
    x, w, b, dy = C.random_data(r)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    ks = [torch.from_numpy(w[l][:, None]).double().requires_grad_(True) for l in range(4)]
    bs = [torch.from_numpy(b[l][None]).double().requires_grad_(True) for l in range(4)] if bias else None
    y = R.dcn_layer(x64, ks, bs, C.ACT_ORACLE[act])
    y.backward(torch.from_numpy(dy).double())
    e = C.cross(x, w, b, dy, act, scales=True)
    pairs = [(e['y'], y.detach().numpy()), (e['dx'], x64.grad.numpy()), (e['dW'], np.stack([k.grad.numpy()[:, 0] for k in ks]))]
    if bias:
        pairs.append((e['db'], np.stack([v.grad.numpy()[0] for v in bs])))
    for a, ref in pairs:
        assert np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # the scales are magnitudes of sums: each is at least the sum it belongs to
    assert (e['s_c'] >= np.abs(e['c']) - 1e-12).all() and (e['s_dW'] >= np.abs(e['dW']) - 1e-12).all() and (e['s_db'] >= np.abs(e['db']) - 1e-12).all()
    assert (e['s_dx'] >= np.abs(e['dx']).max(1) - 1e-12).all()


CENSUS_ROWS = [r for r in T.ROUTES if r['act'] in (C.LINEAR, C.RELU)]


@pytest.mark.parametrize('r', CENSUS_ROWS, ids=[r['name'] for r in CENSUS_ROWS])
def test_census_is_exact(r):
    c = C.make(r, r['act'])
    assert c.params == C.LADDER[0], 'the GPU test draws the first ladder entry'
    assert C.sums_exact(c) < C.EXACT
    assert C.same_bits(C.make(r, r['act'], params=C.LADDER[0]).x, c.x)
    e = C.exact(c)
    for k in ('y', 'c', 'dx', 'dW', 'db'):
        assert (e[k] == np.rint(e[k])).all() and np.abs(e[k]).max() < C.EXACT
    assert np.count_nonzero(e['dW']) > 0 and np.count_nonzero(e['dx']) > 0
    pinned = C.pinned_rows(r['B'])
    assert (np.abs(c.dy[pinned]).min(1) == 1).all() and {0, r['B'] - 1} <= set(pinned.tolist())
    if r['B'] * r['D'] <= 300000:
        # the exact values are the autograd oracle's, bit for bit (integers in fp64)
        x64 = torch.from_numpy(c.x).double().requires_grad_(True)
        ks = [torch.from_numpy(c.w[l][:, None]).double().requires_grad_(True) for l in range(r['L'])]
        bs = [torch.from_numpy(c.b[l][None]).double().requires_grad_(True) for l in range(r['L'])] if c.b is not None else None
        y = R.dcn_layer(x64, ks, bs, C.ACT_ORACLE[r['act']])
        y.backward(torch.from_numpy(c.dy).double())
        assert (y.detach().numpy() == e['y']).all() and (x64.grad.numpy() == e['dx']).all()
        assert all((ks[l].grad.numpy()[:, 0] == e['dW'][l]).all() for l in range(r['L']))
        assert bs is None or all((bs[l].grad.numpy()[0] == e['db'][l]).all() for l in range(r['L']))
    for cap in (2048, 256):                                  # the fast backward's grid at the dcn_grid cap and at occupancy 1
        got = C.restate32(r, c.x, c.w, c.b, c.dy, grid_cap=cap)
        for k in ('y', 'c', 'dx', 'dW', 'db'):
            assert got[k].dtype == np.float32 and C.same_bits(got[k], e[k]), '%s: the fp32 restatement of %s is not exact' % (r['name'], k)


# mistake -> (row, activation of the census, outputs it must change)
PLANTED = {
    'drop_last_row_second_pass': ('fast_d256_l2_lin_b8196', C.LINEAR, ('y', 'dx', 'dW', 'db')),
    'prefetch_clamp': ('fast_d256_l2_lin_b8196', C.LINEAR, ('y', 'c', 'dx', 'dW')),
    'xl_wrong_layer_c': ('fast_d256_l3_lin_b4', C.LINEAR, ('dW',)),
    'xl_wrong_layer_b': ('fast_d256_l3_lin_b4', C.LINEAR, ('dW',)),
    'dx0_without_g': ('fast_d1024_l3_lin_b4', C.LINEAR, ('dx',)),
    'db_before_act_grad': ('templ_d260_l3', C.RELU, ('db',)),
    'slab_left_out': ('fast_d256_l2_lin_b8196', C.LINEAR, ('dW', 'db')),
    'waves_not_combined': ('fast128_b8198_lin', C.LINEAR, ('dx', 'dW')),
}


@pytest.mark.parametrize('mistake', C.MISTAKES)
def test_census_has_teeth(mistake):
    """an fp32 restatement of the kernels with one planted mistake is NOT bit-equal to the census"""
    assert set(PLANTED) == set(C.MISTAKES)
    name, act, changed = PLANTED[mistake]
    r = T.BY_NAME[name]
    c = C.make(r, act, params=C.LADDER[0])
    e = C.exact(c)
    for cap in (2048, 256):
        ok = C.restate32(r, c.x, c.w, c.b, c.dy, grid_cap=cap)
        assert all(C.same_bits(ok[k], e[k]) for k in ('y', 'c', 'dx', 'dW', 'db'))
        bad = C.restate32(r, c.x, c.w, c.b, c.dy, mistake=mistake, grid_cap=cap)
        for k in changed:
            assert not C.same_bits(bad[k], e[k]), '%s (backward grid cap %d): %s is still bit-equal' % (mistake, cap, k)


@pytest.mark.parametrize('r', T.ROUTES, ids=[r['name'] for r in T.ROUTES])
def test_fp32_restatement_under_half_the_bound(r):
    x, w, b, dy = C.random_data(r)
    if r['act'] == C.RELU:
        assert C.min_preact(x, w, b, r['act'])[0] >= C.CLEAR > C.KINK
    ref = C.cross(x, w, b, dy, r['act'], scales=True)
    m = C.margins(C.restate32(r, x, w, b, dy, grid_cap=512), ref, ref)
    assert max(m.values()) <= 0.5, m

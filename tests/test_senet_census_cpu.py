"""CPU: the route table of SENET (tests/_senet_routes.py) and its census (tests/_senet_census.py) are what tests/test_senet_routes_gpu.py takes them for.
  * the Python mirrors of sf_plan and senet_plan equal recnow_senet_fused_route / _fused_grid and recnow_senet_route / _grid (host functions: no
    device needed; the backward's grid follows the device's occupancy and is compared on the GPU) on every row and over a sweep around every threshold;
  * the table reaches every kernel instantiation and every P, and every loop has a one-pass row and a row with a ragged second pass -- from the
    mirror's geometry, not by name;
  * the closed form the scales come from equals oracle/dense_ref.senet_layer under fp64 autograd, and every scale is at least the sum it belongs to;
  * random data: the fp32 restatement of every row stays under half the 1e-5 bound (the condition that the bound is fair, checked with the
    reference alone);
  * census: on every row every sum keeps sum |terms| < 2^24 on the first ladder entry and the fp32 restatement returns the fp64 values to the bit;
    with each planted mistake it does not, and on random data each planted mistake exceeds the bound."""
import itertools

import numpy as np
import pytest

import _senet_census as C
import _senet_routes as T

SMALL = [r for r in T.ROUTES if not r['census_only']]
IDS = [r['name'] for r in SMALL]


def _lib():
    from rec_now_amd import _lib
    return _lib.load()


def test_table_matches_mirror_and_query():
    lib = _lib()
    assert len({r['name'] for r in T.ROUTES}) == len(T.ROUTES)
    for r in T.ROUTES:
        B, F = r['B'], r['F']
        if r['kind'] == 'fused':
            mis = int(bool(r['out_lead']))
            assert lib.recnow_senet_fused_route(0, B, F, r['D'], r['M'], mis) == r['fwd'] == T.fused_route(0, B, F, r['D'], r['M'], mis), r['name']
            assert lib.recnow_senet_fused_route(1, B, F, r['D'], r['M'], 0) == r['bwd'] == T.fused_route(1, B, F, r['D'], r['M'], 0), r['name']
            assert lib.recnow_senet_fused_grid(0, B, F, r['D'], r['M'], mis) == T.fused_grid(0, B, F, r['D'], r['M'], mis), r['name']
            assert lib.recnow_senet_fused_supported(F, r['D'], r['M']) == 1
        else:
            total = sum(r['dims'])
            for mode in (T.SQUEEZE, T.SCALE, T.DW, T.DX):
                assert lib.recnow_senet_route(mode, B, F, total, r['ud']) == r['code'] == T.senet_route(mode, B, F, total, r['ud']), r['name']
                assert lib.recnow_senet_grid(mode, B, F, total, r['ud']) == T.senet_grid(mode, B, F, total, r['ud']), r['name']


FUSED_F = (1, 2, 7, 8, 9, 15, 16, 17, 24, 32, 56, 63, 64, 65)
FUSED_D = (3, 4, 5, 8, 12, 16, 20, 32, 64, 128, 256, 512, 1024, 1028)
FUSED_M = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65)
FUSED_B = (0, 1, 4, 5, 8, 9, 8191, 8192, 8193, 8197, 16383, 16384, 16385, 16395, 1 << 20)


def _fused_sweep():
    for F, D, M, B in itertools.product(FUSED_F, FUSED_D, FUSED_M, FUSED_B):
        for which in (0, 1):
            for mis in (0, 1):
                yield which, B, F, D, M, mis


def _unfused_sweep():
    totals = sorted({t + o for t in (4, 8, 16, 256, 382, 383, 384, 385, 1000, 6143, 6144, 12286, 12287, 12288, 12289, 20000) for o in (0,)} | {1, 2, 6, 30, 260})
    for total in totals:
        for F in (1, 2, 3, 5, 65):
            for ud in sorted({0, 4, 5, 8, 12, 16, 20, 32, 64, 128, 256, 260, 512} | ({total // F} if total % F == 0 else set())):
                for B in (0, 1, 3, 4, 5, 131072, 131073, 1048576, 1048578):
                    for mode in (0, 1, 2, 3):
                        yield mode, B, F, total, ud


def test_mirror_matches_query_over_sweep():
    lib = _lib()
    n = 0
    for a in _fused_sweep():
        assert lib.recnow_senet_fused_route(*a) == T.fused_route(*a), a
        if a[0] == 0:
            assert lib.recnow_senet_fused_grid(*a) == T.fused_grid(*a), a
        n += 1
    for a in _unfused_sweep():
        assert lib.recnow_senet_route(*a) == T.senet_route(*a), a
        assert lib.recnow_senet_grid(*a) == T.senet_grid(*a), a
        n += 1
    # every (F, M) at the instantiation thresholds of the backward, and every M at the P thresholds of both forwards
    for F in range(1, 65):
        for M in range(1, 65):
            assert lib.recnow_senet_fused_route(1, 5, F, 4, M, 0) == T.SF_BWD * 100000 + T.nacc_of(F, M)
    for M in range(1, 65):
        assert lib.recnow_senet_fused_route(0, 5, 8, 16, M, 0) == T.f8(T.sf_split(8, M), 0) and lib.recnow_senet_fused_route(0, 5, 8, 16, M, 1) == T.f4(T.sf_split(4, M))
    assert [T.sf_split(4, M) for M in (8, 9, 16, 17, 32, 33, 64)] == [8, 4, 4, 2, 2, 1, 1] and [T.sf_split(8, M) for M in (4, 5, 8, 9, 16, 17)] == [8, 4, 4, 2, 2, 1]
    assert n > 100000
    # the tile thresholds themselves
    assert [T.tile_rows(t) for t in (383, 384, 1000, 12287, 12288)] == [32, 31, 12, 1, 0]
    assert lib.recnow_senet_route(0, 3, 2, 12288, 0) == T.EUNSUPPORTED and lib.recnow_senet_route(0, 3, 3072, 12288, 4) == T.SENET_UNIFORM * 100000 + 1
    # empty calls and invalid arguments
    assert lib.recnow_senet_route(2, 0, 3, 6, 0) == 0 and lib.recnow_senet_fused_route(1, 0, 3, 8, 2, 0) == 0 and lib.recnow_senet_fused_grid(1, 0, 3, 8, 2, 0) == 0
    for bad in ((4, 5, 3, 6, 0), (-1, 5, 3, 6, 0), (0, -1, 3, 6, 0), (0, 5, 0, 6, 0), (0, 5, 3, 0, 0), (0, 5, 3, 6, -4)):
        assert lib.recnow_senet_route(*bad) == -1 == T.senet_route(*bad) == lib.recnow_senet_grid(*bad), bad
    for bad in ((2, 5, 3, 8, 2, 0), (0, -1, 3, 8, 2, 0), (0, 5, 3, 8, 2, 2), (1, 5, 3, 8, 2, -1)):
        assert lib.recnow_senet_fused_route(*bad) == -1 == T.fused_route(*bad), bad
    assert lib.recnow_senet_fused_route(0, 5, 65, 4, 2, 0) == T.EUNSUPPORTED == lib.recnow_senet_fused_route(1, 5, 3, 128, 65, 0)


def test_table_reaches_every_instantiation_and_every_split():
    """from the codes and the mirror's geometry, not by name"""
    fused = [r for r in T.ROUTES if r['kind'] == 'fused']
    geo = {r['name']: T.geometry(r) for r in T.ROUTES}
    assert {(g['f']['family'], g['f']['P']) for n, g in geo.items() if 'f' in g} == {(T.SF_FWD4, p) for p in (1, 2, 4, 8)} | {(T.SF_FWD8, p) for p in (1, 2, 4, 8)}
    assert {g['b']['nacc'] for g in geo.values() if 'b' in g} == set(T.NACCS)
    assert {(g['b']['P']) for g in geo.values() if 'b' in g} == {1, 2, 4, 8}
    assert {r['fwd'] % 10 for r in fused if r['fwd'] // 100000 == T.SF_FWD8} == {0, 1}                  # with and without the LDS grant
    assert {g['f']['Q'] for g in geo.values() if 'f' in g and g['f']['family'] == T.SF_FWD4} == {1, 2, 4, 8, 16}
    assert {r['F'] * r['D'] // 4 == 256 for r in fused if r['fwd'] // 100000 == T.SF_FWD4} == {True, False}
    assert any(r['F'] == 1 for r in fused) and any(r['D'] == 16 and r['F'] % 8 for r in fused)
    assert any(r['out_lead'] and T.sf8_ok(r['F'], r['D'], r['M']) and r['fwd'] // 100000 == T.SF_FWD4 for r in fused)
    assert {r['F'] for r in fused if r['fwd'] // 100000 == T.SF_FWD8} >= {8, 16, 64}
    assert {r['B'] for r in fused if r['fwd'] // 100000 == T.SF_FWD4} >= {1, 3, 5} and {r['B'] for r in fused if r['fwd'] // 100000 == T.SF_FWD8} >= {1, 7, 9}
    assert any(r['fwd'] // 100000 == T.SF_FWD8 and 8 * r['M'] > 256 and (8 * r['M']) % 256 for r in fused)      # a second, ragged round of the h loop
    # both sides of every change of the backward's instantiation, found by the mirror
    nouts = {2 * r['F'] * r['M'] + r['M'] + r['F']: r for r in fused}
    for n, lo, _, hi, _ in T.bwd_edges():
        assert lo <= 256 * n < hi and nouts[lo]['bwd'] % 100000 == n and nouts[hi]['bwd'] % 100000 == T.NACCS[T.NACCS.index(n) + 1], (n, lo, hi)
        assert not any(lo < 2 * F * M + M + F < hi for F in range(1, 65) for M in range(1, 65))
    assert 768 in nouts and (nouts[768]['F'], nouts[768]['M']) == (14, 26) and 8320 in nouts and [e[1] for e in T.bwd_edges()][0] == 768
    # every activation code in both positions in each of the three kernel families (the backward runs on every fused row)
    for fam in (T.SF_FWD4, T.SF_FWD8):
        rows = [r for r in fused if r['fwd'] // 100000 == fam]
        assert {r['acts'][0] for r in rows} == {0, 1, 2, 3} == {r['acts'][1] for r in rows}, fam
    # the four bias combinations on both forwards
    for fam in (T.SF_FWD4, T.SF_FWD8):
        assert {(r['b1'], r['b2']) for r in fused if r['fwd'] // 100000 == fam} == {(False, False), (True, False), (False, True), (True, True)}
    assert {r['view'] for r in fused} == {None, 'field', 'dout'}
    # unfused: every Q of the uniform kernel, the tile kernel at R = 32, 31, 12 and 1 with B no multiple of R
    uni = [r for r in T.ROUTES if r['kind'] == 'unfused' and r['code'] // 100000 == T.SENET_UNIFORM]
    tile = [r for r in T.ROUTES if r['kind'] == 'unfused' and r['code'] // 100000 == T.SENET_TILE]
    assert {r['code'] % 100000 for r in uni} == {1, 2, 4, 8, 16, 32, 64}
    assert any(r['F'] == 65 for r in uni) and any(r['F'] * r['dims'][0] // 4 > 256 for r in uni) and all(r['B'] % 4 for r in uni)
    assert all(geo[r['name']]['u']['items'] % 256 for r in uni)
    assert all(r['layer'] for r in uni if not r['census_only']), 'the uniform rows are what the layer sends there'
    assert {r['code'] % 100000 for r in tile} == {32, 31, 12, 1}
    assert all(any(r['code'] % 100000 == R and r['B'] % R for r in tile) for R in (32, 31, 12))
    assert any(r['ud'] == 0 and len(set(r['dims'])) == 1 and r['dims'][0] % 4 == 0 for r in tile)
    assert any(len(set(r['dims'])) == 1 and r['dims'][0] % 4 for r in tile)
    assert {tuple(r['dims']) for r in tile} >= {(1, 2, 3), (5,), (4, 8, 4, 32, 1), (6,) * 5}
    assert sum(T.TOTAL_UNSUPPORTED) == 12288 and T.senet_route(0, 3, 2, 12288, 0) == T.EUNSUPPORTED


def test_every_loop_has_a_one_pass_and_a_ragged_two_pass_row():
    seen = {}
    for r in T.ROUTES:
        for d, e in T.geometry(r, occ=64).items():                # the largest backward grid any device gives, min(ceil(B / 4), 2048): the fewest passes
            n, per = (e['items'], e['per']) if 'items' in e else (r['B'], e['stride'])
            seen.setdefault((r['kind'], d, e['family']), set()).add('one' if n <= per else 'ragged' if n % per else 'whole')
    want = [('fused', 'f', T.SF_FWD4), ('fused', 'f', T.SF_FWD8), ('fused', 'b', T.SF_BWD), ('unfused', 'u', T.SENET_UNIFORM), ('unfused', 'u', T.SENET_TILE)]
    assert set(seen) == set(want)
    for key in want:
        assert {'one', 'ragged'} <= seen[key], (key, seen[key])
    # the shapes of the issue: workgroup 0 a whole second step, workgroup 1 a ragged one, the rest none
    g = T.geometry(T.BY_NAME['sf4_two_pass'])
    assert g['f']['grid'] == 2048 and g['f']['passes'] == 2 and 8197 - g['f']['stride'] == 4 + 1 and g['b']['passes'] >= 2
    assert T.geometry(T.BY_NAME['sf4_two_pass'], occ=1)['b']['passes'] == 9 and T.geometry(T.BY_NAME['sf4_two_pass'], occ=64)['b']['passes'] == 2
    g = T.geometry(T.BY_NAME['sf8_two_pass'])
    assert g['f']['grid'] == 2048 and g['f']['passes'] == 2 and 16395 - g['f']['stride'] == 8 + 3
    g = T.geometry(T.BY_NAME['uni_two_pass'])['u']
    assert g['grid'] == 16384 and g['passes'] == 2 and g['items'] - g['per'] == 16
    g = T.geometry(T.BY_NAME['tile_two_pass'])['u']
    assert g['grid'] == 4096 and g['passes'] == 2 and 131109 - g['stride'] == 32 + 5


# ---- closed form ------------------------------------------------------------------------------------------------------------------------------------------
CLOSED = [dict(kind='fused', name='closed %s %s %s' % (T.ACT_NAMES[a1], T.ACT_NAMES[a2], 'bias' if b else 'no bias'), B=23, F=len(dims), dims=dims, M=3, acts=(a1, a2),
               b1=b, b2=b, census_only=False) for (a1, a2), b, dims in zip(T._ACTS, [True, False] * 8, [[1, 2, 3], [8] * 4, [5], [4, 8, 4, 32, 1]] * 4)]


@pytest.mark.parametrize('r', CLOSED, ids=[r['name'] for r in CLOSED])
def test_closed_form_is_the_autograd_oracle(r):
    d = C.random_data(r)
    assert C.kink_clearance(d, r['acts']) >= C.CLEAR > C.KINK
    e, ref = C.senet(d, r['acts'], scales=True), C.oracle(d, r['acts'])
    for k in C.outputs(r, 'layer'):
        a, b, s = C._flat(e[k]), C._flat(ref[k]), C._flat(e['s_' + k])
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), k
        assert (s >= np.abs(a) - 1e-12).all(), k                 # the scales are magnitudes of sums: each is at least the sum it belongs to
    for k in ('sq', 'h', 'w'):
        assert (e['s_' + k] >= np.abs(e[k]) - 1e-12).all(), k


# ---- census -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', SMALL, ids=IDS)
def test_census_is_exact(r):
    d, p = C.make(r)
    assert p in C.LADDER and C.make(r)[1] == p                  # the GPU test draws the same entry: make() walks the ladder there too
    unit = C.denominator(r['dims'])
    assert C.largest_sum(r, d) < C.EXACT
    assert all((np.asarray(x) != 0).all() for x in d['x']) and (d['W1'] != 0).all() and (d['W2'] != 0).all()
    acts = C.census_acts(r['acts'])
    assert set(acts) <= {T.LINEAR, T.RELU}
    e = C.model(r, d, acts)
    for k in (C.FUSED_OUT if r.get('layer_census', True) else ()):
        v = C._flat(e[k])
        assert (v * unit == np.rint(v * unit)).all() and np.abs(v).max() * unit < C.EXACT, k
    if r['B'] * sum(r['dims']) <= 300000:
        ref = C.oracle(d, acts)                                   # the exact values are the autograd oracle's (integers in fp64)
        for k in (k for k in C.outputs(r, 'layer') if k in ref):
            assert (C._flat(ref[k]) == C._flat(e[k])).all(), k
    # informative: rows differ from row to row and fields from field to field, the pinned rows carry gradient
    if r['B'] > 1:
        assert (np.abs(np.diff(e['out'], axis=0)).sum(1) != 0).mean() > 0.9
    if r['F'] > 2:
        assert (np.diff(e['sq'], axis=1) != 0).mean() > 0.5
    assert (d['dout'][T.pinned_rows(r)] != 0).all() and np.count_nonzero(C._flat(e['dx'])) > 0
    if r['kind'] == 'fused':
        got = C.model(r, d, acts, np.float32, restate=True)
        for k in C.FUSED_OUT:
            assert np.asarray(got[k][0] if isinstance(got[k], list) else got[k]).dtype == np.float32, k
            assert C.bits_equal(got[k], e[k]), '%s: the fp32 restatement of %s is not exact' % (r['name'], k)
    else:
        ee, got = C.entry(r, d), C.entry(r, d, np.float32, restate=True)
        for k in C.ENTRY_OUT:
            v = C._flat(ee[k])
            assert (v * unit == np.rint(v * unit)).all() and C.bits_equal(got[k], ee[k]), '%s: the fp32 restatement of %s is not exact' % (r['name'], k)


def test_census_of_the_large_uniform_row_is_exact_by_its_bounds():
    """uni_two_pass is 67 M floats a tensor: no fp64 array of that size is built.  Its sums are one field row each: at most D terms of at most
    xmax x gmax, and dout w + dsq / D of three small integers -- below 2^24 by arithmetic, so fp32 numpy in any order is exact."""
    r = T.BY_NAME['uni_two_pass']
    xmax, wmax, gmax = C.LADDER[0]
    D = r['dims'][0]
    assert r['census_only'] and not r['layer'] and C.width_lcm(r['dims']) == 1 and D & (D - 1) == 0
    assert max(D * xmax, D * xmax * gmax, xmax * wmax, gmax * wmax + gmax) < C.EXACT
    assert r['B'] * sum(r['dims']) == 67108992


# mistake -> rows that reach the code, outputs it must change
PLANTED = {
    'prefetch_not_advanced': [('sf4_two_pass', ('out', 'sq', 'dx', 'dW1')), ('sf8_two_pass', ('out', 'sq', 'dx'))],
    'rows_past_B_counted': [('sf4_two_pass', ('dW1', 'dW2', 'db2')), ('sf4_q2', ('dW1', 'db1'))],
    'half_butterfly': [('sf4_q8_full', ('sq', 'out', 'dx')), ('uni_q16', ('e_sq', 'e_dw'))],
    'dsq_over_total': [('sf4_q4', ('dx',)), ('tile_123', ('e_dx',))],
    'fwd8_last_pass_dropped': [('sf8_m3', ('sq', 'out')), ('sf8_grant', ('sq', 'out'))],
    'bias_grad_skipped': [('sf4_m9', ('db1',)), ('sf8_m5', ('db1',))],
    'tile_offset_shifted': [('tile_mixed', ('e_dw', 'e_dx')), ('tile_6x5', ('e_dw', 'e_dx'))],
    'act2_grad_from_h': [('sf4_m9', ('dx', 'dW2')), ('sf8_m5', ('dx', 'dW2'))],
    'last_slot_not_stored': [('bwd_n8320', ('db2',)), ('bwd_n768', ('db2',))],
}


@pytest.mark.parametrize('mistake', C.MISTAKES)
def test_census_has_teeth(mistake):
    """an fp32 restatement of the kernels with one planted mistake is NOT bit-equal to the census, and on random data it is over the bound"""
    assert set(PLANTED) == set(C.MISTAKES) and len(C.MISTAKES) == 9
    over = 0
    for name, changed in PLANTED[mistake]:
        r = T.BY_NAME[name]
        d, _ = C.make(r)
        acts = C.census_acts(r['acts'])
        e = C.compute(r, d, acts)
        ok, bad = C.compute(r, d, acts, np.float32, True), C.compute(r, d, acts, np.float32, True, mistake)
        assert all(C.bits_equal(ok[k], e[k]) for k in C.outputs(r))
        for k in changed:
            assert not C.bits_equal(bad[k], e[k]), '%s on %s: %s is still bit-equal' % (mistake, name, k)
        rd = C.random_data(r)
        ref = C.compute(r, rd, scales=True)
        m = C.margins(changed, C.compute(r, rd, None, np.float32, True, mistake), ref, ref)
        over += max(m.values()) > 1.0
    assert over >= 1, '%s stays inside the random-data bound on every row' % mistake


WORST = {}


@pytest.mark.parametrize('r', SMALL, ids=IDS)
def test_fp32_restatement_under_half_the_bound(r):
    d = C.random_data(r)
    assert C.kink_clearance(d, r['acts']) >= C.CLEAR > C.KINK
    ref = C.compute(r, d, scales=True)
    m = C.margins(C.outputs(r), C.compute(r, d, None, np.float32, True), ref, ref)
    for k, v in m.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert max(m.values()) <= 0.5, m


def test_worst_restatement_margins_are_reported():
    print('largest fraction of the bound in the fp32 restatement: ' + '  '.join('%s %.4f' % kv for kv in sorted(WORST.items())))
    assert all(v <= 0.5 for v in WORST.values())

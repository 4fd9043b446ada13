"""The DCN-v2 layer census (tests/_mix_census.py) has teeth, without a GPU: every row of the layer route table (tests/_mix_routes.py) gets census
data whose every product stays inside the 2^24-unit window -- in the plain and in the bf16x3 split form, every operand with at most 16
significant bits -- so fp32 restatements of the layer in three summation orders equal the exact result bit for bit; and every listed kernel
mistake that applies to the row moves at least one checked output."""
import numpy as np
import pytest

import _mix_census as M
from _mix_routes import ROUTES, spec
from _split_census import bf16_split

_CACHE = {}


def _census(r):
    key = tuple(sorted(spec(r).items()))
    if key not in _CACHE:
        _CACHE[key] = M.make(**spec(r))
    c = _CACHE[key]
    assert c.params == r['census'], '%s: the table says census parameters %r, the ladder picks %r' % (r['name'], r['census'], c.params)
    return c


def _same(what, got, want):
    got = np.asarray(got, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1).view(np.int32) != want.astype(np.float32).reshape(-1).view(np.int32))
    assert bad.size == 0, '%s: %d of %d differ, first flat %d: %r vs %r' % (what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]],
                                                                          want.reshape(-1)[bad[0]])


@pytest.mark.parametrize('r', ROUTES, ids=[r['name'] for r in ROUTES])
def test_row_census_is_exact(r):
    c = _census(r)          # M.make has checked the window (plain and split form), the 16-bit operands and the fp32 intermediates
    for ai, ao in ((M.LINEAR, M.LINEAR), (M.RELU, M.RELU)):
        want = M.expected(c, ai, ao)
        names = list(want)
        assert (r['entry'] == 'score') == ('scores' in names) and ('dx' in names) == bool(r['need_dx'])
        for order, mm in M.ORDERS.items():
            got = M.restate(c, ai, ao, mm=mm, dtype=np.float32)
            for k in names:
                _same('%s %s act %d' % (r['name'], order, ai), got[k], want[k])
        # the census is not degenerate: most outputs and (LINEAR) every gradient carry nonzero values; a deep sparse RELU stack may zero a
        # whole lower-layer gradient (its LINEAR census checks that gradient)
        for k in names if ai == M.LINEAR else ():
            if not (k.startswith('dK') and r['N'] == 1):           # one expert: dlogits = G (dG - <G, dG>) = 0
                assert np.count_nonzero(want[k]) > 0, '%s: %s is all zero' % (r['name'], k)
        out = want['scores'] if 'scores' in want else want['y']
        assert np.count_nonzero(out) > 0.5 * out.size


@pytest.mark.parametrize('r', ROUTES, ids=[r['name'] for r in ROUTES])
def test_row_respects_the_split_condition(r):
    """Every operand of every product has at most 16 significant bits: the third piece of the split model (bf16_split) is zero."""
    c = _census(r)
    res = M.restate(c, M.RELU, M.RELU, keep=True)
    k = res['_keep']
    for name, arrs in (('x', k['x']), ('T1', k['T1']), ('H2', k['H2']), ('O', k['O']), ('g', k['g'])):
        for a in arrs:
            u = np.unique(a.astype(np.float32))
            assert not np.count_nonzero(bf16_split(u)[2]), '%s has values with more than 16 significant bits' % name
    for name, v in c.inp.items():
        for a in (v if isinstance(v, list) else [v]):
            assert not np.count_nonzero(bf16_split(np.unique(a))[2]), name


@pytest.mark.parametrize('r', ROUTES, ids=[r['name'] for r in ROUTES])
def test_row_catches_every_mutation(r):
    c = _census(r)
    s = spec(r)
    clean = M.restate(c, M.RELU, M.RELU)
    for mut, (what, applies) in M.MUTATIONS.items():
        if not applies(s):
            continue
        bad = M.restate(c, M.RELU, M.RELU, mut=mut)
        moved = [k for k in clean if not np.array_equal(clean[k], bad[k])]
        assert moved, '%s: mutation %r (%s) changes no checked output' % (r['name'], mut, what)


def test_split3_is_the_split_model():
    x = (np.random.default_rng(0).standard_normal(200000) * np.exp2(np.random.default_rng(1).integers(-30, 30, 200000))).astype(np.float32)
    for a, b in zip(M.split3(x), bf16_split(x)):
        assert np.array_equal(a, b)


def test_window_shrinks_the_data_where_needed():
    """a deep stack at D = 1024 does not fit the first data parameters: the helper shrinks them, and the result holds the invariant"""
    c = M.make(B=512, D=1024, S=64, N=2, L=4)
    assert c.params != M.LADDER[0]
    assert max(M.units(c, M.RELU, M.RELU).split_units.values()) < M.WINDOW
    c = M.make(B=256, D=128, S=64, N=2, L=1)
    assert c.params == M.LADDER[0]


def test_invariant_is_enforced():
    c = M.make(B=256, D=128, S=64, N=2, L=1)
    c.inp['x'] = c.inp['x'] * np.float32(4096.0)
    with pytest.raises(AssertionError):
        M.units(c, M.LINEAR, M.LINEAR)

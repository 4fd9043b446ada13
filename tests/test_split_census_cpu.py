"""The planted-piece census (tests/_split_census.py) has teeth, without a GPU: the correct six-term split product of its inputs, accumulated in
fp32, is exactly the expected output, and every way of getting the arithmetic subtly wrong -- a dropped or doubled term, pieces 2 and 3
swapped, the piece-3 plane of the neighbouring row -- moves at least one output by >= 2^-20 of itself."""
import numpy as np
import pytest

import _split_census as SC

SHAPE = dict(M=64, N=128, K=1024)


def _present(case):
    """Pieces that are nonzero in a sub-case: (pieces of A', pieces of B)."""
    return {'a': ({1, 2, 3}, {1}), 'b': ({1}, {1, 2, 3}), 'c': ({1, 2}, {1, 2}), 'd': ({1, 2, 3}, {1})}[case]


def _mutations():
    """name -> (weights, transform of the pieces (a, b) -> (a, b), (A pieces, B pieces) it touches)"""
    m = {}
    for t in SC.TERMS:
        m['drop a%db%d' % t] = ({**dict.fromkeys(SC.TERMS, 1.0), t: 0.0}, None, ({t[0]}, {t[1]}))
        m['double a%db%d' % t] = ({**dict.fromkeys(SC.TERMS, 1.0), t: 2.0}, None, ({t[0]}, {t[1]}))
    # a plain exchange of pieces 2 and 3 only shows in a2b2 (a2b1 + a3b1 is symmetric in them); reading one plane for the other shows everywhere
    m['A pieces 2 <-> 3'] = (None, lambda a, b: ([a[0], a[2], a[1]], b), ({2, 3}, set()))
    m['B pieces 2 <-> 3'] = (None, lambda a, b: (a, [b[0], b[2], b[1]]), (set(), {2, 3}))
    m['A piece 2 read from plane 3'] = (None, lambda a, b: ([a[0], a[2], a[2]], b), ({2, 3}, set()))
    m['A piece 3 read from plane 2'] = (None, lambda a, b: ([a[0], a[1], a[1]], b), ({2, 3}, set()))
    m['B piece 2 read from plane 3'] = (None, lambda a, b: (a, [b[0], b[2], b[2]]), (set(), {2, 3}))
    m['B piece 3 read from plane 2'] = (None, lambda a, b: (a, [b[0], b[1], b[1]]), (set(), {2, 3}))
    m['A piece 3 of the next row'] = (None, lambda a, b: ([a[0], a[1], np.roll(a[2], -1, axis=0)], b), ({3}, set()))
    m['B piece 3 of the next column'] = (None, lambda a, b: (a, [b[0], b[1], np.roll(b[2], -1, axis=1)]), (set(), {3}))
    return m


@pytest.fixture(scope='module', params='abcd')
def census(request):
    return SC.make(seed=ord(request.param), case=request.param, **SHAPE)


def test_six_term_product_is_exact(census):
    c = census
    assert c.T == (1 if c.case == 'c' else 2)
    np.testing.assert_array_equal(SC.emulate(c.a, c.b).astype(np.float64), c.C)
    assert np.count_nonzero(c.C) == c.C.size                   # every output has a value to get wrong
    # the stored fp32 operands are the census (A' = A * A2 exactly), and the side product is exact too
    Ap = c.A.astype(np.float64) * (c.A2.astype(np.float64) if c.A2 is not None else 1.0)
    np.testing.assert_array_equal(Ap, c.a.sum(0))
    np.testing.assert_array_equal((Ap.astype(np.float32) @ c.Bx).astype(np.float64), c.Cx)
    assert np.count_nonzero(c.Cx) == c.Cx.size
    # the dropped terms are zero: the exact fp32 product of the same inputs is the same number
    np.testing.assert_array_equal(SC.emulate([Ap, 0 * Ap, 0 * Ap], [c.B.astype(np.float64), 0 * c.b[0], 0 * c.b[0]],
                                             weights={(1, 1): 1.0}).astype(np.float64), c.C)


def test_census_covers_the_tile_and_the_k_positions(census):
    c = census
    K = SHAPE['K']
    used = np.sort(c.pos.reshape(-1))
    assert used[0] == 0 and used[-1] == K - 1
    tiles = used // 16
    assert set((used % 16) // 8) == {0, 1}                     # both k-halves of a k-tile
    assert set(tiles % 2) == {0, 1}                            # both members of a PAIR couple
    assert len(set(tiles)) == K // 16                          # every k-tile: the first and last of any chunk or slab


@pytest.mark.parametrize('name', sorted(_mutations()))
def test_every_mutation_is_caught(census, name):
    c = census
    w, tf, (ta, tb) = _mutations()[name]
    a, b = (tf(list(c.a), list(c.b)) if tf else (c.a, c.b))
    C = SC.emulate(a, b, w).astype(np.float64)
    rel = np.abs(C - c.C) / np.abs(c.C)
    pa, pb = _present(c.case)
    # a mutation that touches only pieces which are zero in this sub-case is harmless here (another sub-case catches it); one that touches a
    # planted piece must show
    if name.startswith(('drop', 'double')):
        live = bool(ta & pa) and bool(tb & pb)
    elif '<->' in name:
        live = c.case == 'c'
    else:
        live = bool(ta & pa) or bool(tb & pb)
    if live:
        assert rel.max() >= 2.0 ** -20, (name, rel.max())
    else:
        assert rel.max() == 0.0


def test_every_mutation_is_caught_by_some_sub_case():
    cs = [SC.make(seed=ord(k), case=k, M=32, N=128, K=512) for k in 'abcd']
    for name, (w, tf, _) in _mutations().items():
        hit = False
        for c in cs:
            a, b = (tf(list(c.a), list(c.b)) if tf else (c.a, c.b))
            hit |= bool((np.abs(SC.emulate(a, b, w).astype(np.float64) - c.C) >= 2.0 ** -20 * np.abs(c.C)).any())
        assert hit, name


@pytest.mark.parametrize('K,kv', [(144, 130), (144, 144), (8192, None)])
def test_census_at_the_other_depths(K, kv):
    """Short K with a zero-padded depth (every used k below k_valid), and a long K whose used positions spread over the whole depth."""
    c = SC.make(M=128, N=256, K=K, case='a', seed=5, k_valid=kv)
    assert c.pos.max() < (kv or K)
    np.testing.assert_array_equal(SC.emulate(c.a, c.b).astype(np.float64), c.C)
    if kv:
        assert not c.A[:, kv:].any() and not c.B[kv:].any()


def test_host_split_saturates_at_the_top_of_the_fp32_range():
    """bf16_split mirrors spl_split2: a finite |x| >= 3.3961e38 (which rounds to inf in bf16) gives piece 1 = +-bf16_max and finite pieces
    that sum back to x; inf and NaN stay non-finite."""
    x = np.array([3.3961e38, -3.4e38, np.finfo(np.float32).max, 3.3e38, np.inf, -np.inf, np.nan], np.float32)
    p = SC.bf16_split(x)
    fin = np.isfinite(x)
    assert np.isfinite(np.array(p)[:, fin]).all()
    assert np.abs(p[0][fin][:3]).max() == 3.3895313892515355e38
    err = np.abs(p[0][fin].astype(np.float64) + p[1][fin] + p[2][fin] - x[fin].astype(np.float64))
    assert (err <= 2.0 ** -24 * np.abs(x[fin].astype(np.float64))).all()
    assert not np.isfinite(p[0][~fin] + p[1][~fin] + p[2][~fin]).any()

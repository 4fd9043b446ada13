"""The exact census (tests/_exact_census.py) has teeth, without a GPU: every row of the exact-fp32 route table (tests/_gemm_routes.py) gets a
census whose products stay inside the 2^24-unit window and whose epilogue steps are exact in fp32, and every listed way of getting a product
subtly wrong moves at least one census output."""
import numpy as np
import pytest

import _exact_census as E
from _gemm_routes import ROUTES


def _census_spec(spec, extra):
    s = dict(E.SPEC_DEFAULTS)
    s.update(spec)
    mt, nt = extra.get('tile', (1, 1))
    return dict(s, M=s['M'] // mt, N=s['N'] // nt)


@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_route_census_is_exact(route):
    name, _, spec, extra, _ = route
    c = E.make(_census_spec(spec, extra))
    worst, _ = E.term_units(c)
    assert worst < E.WINDOW
    C, Cx, aso = E.expected(c, E.LINEAR, check=True)
    z = E.preactivation(c)
    assert np.count_nonzero(z) > 0.9 * z.size                 # (an emul ACTGRAD of RELU zeroes half of C itself)
    assert Cx is None or np.count_nonzero(Cx) > 0.5 * Cx.size


def test_window_shrinks_values_where_needed():
    """ACTGRAD with TANH factors (1 - j^2 / 64) at K = 65536 cannot keep vmax 7 inside 2^24 units: the helper shrinks the values."""
    c = E.make(M=64, N=64, K=65536, a_mode=E.ACTGRAD, a_act=E.TANH)
    assert c.vmax < 7 and E.term_units(c)[0] < E.WINDOW
    c = E.make(M=64, N=64, K=4096, a_mode=E.ACTGRAD, a_act=E.TANH)
    assert E.term_units(c)[0] < E.WINDOW
    c = E.make(M=64, N=64, K=384)
    assert c.vmax == 7


def test_invariant_is_enforced():
    """A census whose sums leave the window is refused: vmax 7 integers at K = 2^19 cannot be made exact by shrinking to 1 either."""
    with pytest.raises(AssertionError):
        E.make(M=8, N=8, K=1 << 24 >> 4, a_mode=E.ACTGRAD, a_act=E.SIGMOID)


def _moved(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b))


BASE = dict(M=128, N=96, K=77, bias=1, e_mode=E.MUL, accumulate=1, act_cols=50)


@pytest.fixture(scope='module')
def base():
    return E.make(BASE)


def test_mutations_move_an_output(base):
    c = base
    C = E.expected(c)[0]
    z = E.preactivation(c)

    def with_product(P):
        r = E.Census()
        r.spec, r.stored, r.Ae, r.Be = c.spec, c.stored, c.Ae, c.Be
        zz = P + c.stored['bias']
        return E.finish(r, E.apply_act(r, zz, E.LINEAR))
    Ae, Be = c.Ae, c.Be
    keep = lambda ks: Ae[:, :, ks] @ Be[:, ks, :]      # noqa: E731
    K = c.spec['K']
    allk = np.arange(K)
    muts = {
        'dropped k-tile': with_product(keep(allk[(allk < 32) | (allk >= 64)])),
        'dropped last k-pair of a ragged K': with_product(keep(allk[allk < K - 1])),
        'dropped single k': with_product(keep(allk[allk != 40])),
        'row shifted by one inside a tile': np.concatenate([C[:, 1:2], C[:, :1], C[:, 2:]], 1),
        'column shifted by one inside a tile': np.concatenate([C[:, :, 1:2], C[:, :, :1], C[:, :, 2:]], 2),
        'bias of the neighbouring column': E.finish(c, E.apply_act(c, Ae @ Be + np.roll(c.stored['bias'], 1, axis=2), E.LINEAR)),
        'emul of the neighbouring column': (z * np.roll(c.stored['E'], 1, axis=2)) + c.stored['C0'],
        'missing accumulate': z * c.stored['E'],
    }
    for k, v in muts.items():
        assert _moved(v, C), k


@pytest.mark.parametrize('act', [E.RELU, E.TANH, E.SIGMOID])
def test_actgrad_of_another_activation_moves(act):
    for side in ('A', 'B'):
        kw = dict(M=64, N=64, K=256, a_mode=E.ACTGRAD, a_act=act) if side == 'A' else dict(M=64, N=64, K=256, b_mode=E.ACTGRAD, b_act=act)
        c = E.make(kw)
        C = E.expected(c)[0]
        for other in (E.RELU, E.TANH, E.SIGMOID):
            if other == act:
                continue
            key = 'a_act' if side == 'A' else 'b_act'
            o = E.Census()
            o.spec, o.stored = dict(c.spec, **{key: other}), c.stored
            assert _moved(E.effective(o.spec, o.stored, 'A') @ E.effective(o.spec, o.stored, 'B'), C), (side, act, other)
    # the emul form
    c = E.make(M=64, N=64, K=256, e_mode=E.ACTGRAD, e_act=act)
    C = E.expected(c)[0]
    for other in (E.RELU, E.TANH, E.SIGMOID):
        if other != act:
            o = E.Census()
            o.spec, o.stored, o.Ae, o.Be = dict(c.spec, e_act=other), c.stored, c.Ae, c.Be
            assert _moved(E.expected(o)[0], C), ('emul', act, other)


@pytest.mark.parametrize('side', ['A', 'B'])
def test_swapped_outer_index_moves(side):
    kw = dict(M=128, N=128, K=384, ta=0, tb=0)
    kw.update({'a_mode': E.OUTER, 'a_hq': 16} if side == 'A' else {'b_mode': E.OUTER, 'b_hq': 16})
    c = E.make(kw)
    C = E.expected(c)[0]
    first, second = c.stored[side].astype(np.float64), c.stored[side + '2'].astype(np.float64)
    hq, nsec = first.shape[2], second.shape[2]
    cols = np.arange(hq * nsec)
    swapped = second[:, :, cols % nsec] * first[:, :, cols // nsec]       # second[r][c % n2] * first[r][c / n2]
    if side == 'A':
        got = swapped @ c.Be
    else:
        got = c.Ae @ swapped
    assert _moved(got, C)


def test_side_product_column_swap_moves():
    c = E.make(M=128, N=128, K=384, sp_r=2)
    Cx = E.expected(c)[1]
    assert _moved(Cx[:, ::-1], Cx)


def test_rank_update_and_as_out_are_exact():
    c = E.make(M=128, N=128, K=256, eu_r=3, sp_r=2, a_mode=E.MUL, as_out=1, bias=1, accumulate=1)
    C, Cx, aso = E.expected(c, E.RELU, check=True)
    assert aso.shape == c.stored['A'][0].shape and np.count_nonzero(aso) == aso.size
    without = E.finish(c, E.apply_act(c, c.Ae @ c.Be + c.stored['bias'], E.RELU))
    assert _moved(without, C), 'the rank-R update must move the census'


@pytest.mark.parametrize('kc', [256, 8192])
def test_split_slab_twice_or_dropped_moves(kc):
    K = 4 * kc
    c = E.make(M=64, N=64, K=K)
    C = E.expected(c)[0]
    slab = c.Ae[:, :, kc:2 * kc] @ c.Be[:, kc:2 * kc, :]
    assert _moved(C + slab, C) and _moved(C - slab, C)


def test_c_perm_off_by_one_moves():
    c = E.make(M=128, N=128, K=256)
    C = E.expected(c)[0][0]
    s = 64
    good = E.permute_store(C, s)
    M, N = C.shape
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing='ij')
    bad = np.empty(M * N)
    bad[((n // s) * M + m) * s + (n + 1) % s] = C                      # the column inside a group off by one
    assert _moved(bad, good)
    bad2 = np.empty(M * N)
    bad2[((n // s) * M + (m + 1) % M) * s + n % s] = C                  # the row off by one
    assert _moved(bad2, good)

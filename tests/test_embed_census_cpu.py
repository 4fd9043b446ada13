"""The pooled-embedding census (tests/_embed_census.py) has teeth, without a GPU: the backward layouts reach every segment class and every
layout class at every D class, each segment of the main layout is what the table says it is, the forward cases reach every route, the
restated constants are the ones the source defines, the fp64 oracle agrees with an independent dense formulation, and the exact family's sums
fit the fp32 window -- measured on the data, not argued."""
import os

import numpy as np
import pytest

import _embed_census as E
import _embed_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'rec_now_amd', 'csrc', 'embed.hip')


def pinned_constants(text):
    return all(('#define %s %d' % (name, val)) in ' '.join(text.split())
               for name, val in (('EMB_CH', E.EMB_CH), ('EMB_JU', E.EMB_JU), ('EMB_JSHORT', E.EMB_JSHORT)))


def test_constants_match_the_source():
    text = open(SOURCE).read()
    assert pinned_constants(text), 'embed.hip no longer defines EMB_CH 32, EMB_JU 16, EMB_JSHORT 16: rework the layouts of _embed_census.py'
    for name in ('EMB_CH', 'EMB_JU', 'EMB_JSHORT'):           # a retuned constant fails the pin
        assert not pinned_constants(text.replace('#define %s ' % name, '#define %s 1' % name))
    assert 'D <= 16 ? 16 : D <= 32 ? 32 : 64' in text         # LPE
    assert [E.LPE(d) for d in (1, 16, 17, 32, 33, 64, 65, 130)] == [16, 16, 32, 32, 64, 64, 64, 64]
    assert 'per_wave * w > 64 * 1024' in text                 # pool_cfg
    assert E.KEY_NOT_POOLED == -(1 << 63) and '0x8000000000000000ull' in text


@pytest.mark.parametrize('D', E.D_CLASSES)
def test_layouts_reach_every_backward_class(D):
    seg, lay = set(), set()
    for lengths in E.layouts(D):
        cls = E.classify_segments(lengths, D)
        assert len(cls) == len(lengths) and all(c for c in cls)
        seg |= set().union(*cls)
        lay |= E.classify_layout(lengths)
    assert seg == set(E.SEGMENT_CLASSES), (sorted(set(E.SEGMENT_CLASSES) - seg), sorted(seg - set(E.SEGMENT_CLASSES)))
    assert lay == set(E.LAYOUT_CLASSES), (sorted(set(E.LAYOUT_CLASSES) - lay), sorted(lay - set(E.LAYOUT_CLASSES)))
    # both joins from both slots
    for c in ('lane_join_slot0', 'lane_join_slot1', 'wg_join_slot0', 'wg_join_slot1'):
        assert c in seg
    assert len(E.layouts(D)) == len(E.LAYOUT_NAMES)
    # the largest case stays small: no more floats than 12 813 rows of 130
    assert max(sum(lengths) for lengths in E.layouts(D)) * D <= 12813 * 130


@pytest.mark.parametrize('D', E.D_CLASSES)
def test_main_layout_is_what_the_table_says(D):
    m = E.main_layout(D)
    assert sum(m) == E.MAIN_N[E.LPE(D)] and sum(m) % E.EMB_CH == 13
    assert tuple(E.role(c) for c in E.classify_segments(m, D)) == E.MAIN_ROLES
    for i in range(len(m)):                                    # no segment can go: the table (and N) pin each one
        cut = m[:i] + m[i + 1:]
        assert sum(cut) != sum(m) and tuple(E.role(c) for c in E.classify_segments(cut, D)) != E.MAIN_ROLES
    main = set().union(*E.classify_segments(m, D))
    # alone it reaches every class but the ones that need a workgroup join starting on the grid (aligned_layout adds those) and the edges of
    # the unrolled loop (unroll_layout)
    assert set(E.SEGMENT_CLASSES) - main <= {'wg_join_slot0', 'wg_join_ends_at_chunk_end', 'wg_join_even_tail', 'wg_join_lane_tail_15',
                                            'wg_join_lane_no_tail'}
    assert {'lane_join_span_15', 'wg_join_span_16', 'wg_join_unrolled', 'whole_one_chunk'} <= main


def test_classifier_on_hand_cases():
    one = lambda n, pre=0, D=16: E.classify_segments(([pre] if pre else []) + [n], D)[-1]         # noqa: E731
    assert one(32) == {'whole', 'whole_at_chunk_start', 'whole_at_chunk_end', 'whole_one_chunk'}
    assert one(33) == {'lane_join', 'lane_join_slot0'}
    assert one(2, pre=31) == {'lane_join', 'lane_join_slot1'}
    assert one(33, pre=31) == {'lane_join', 'lane_join_slot1', 'lane_join_ends_at_chunk_end'}
    assert one(15 * 32 + 1) >= {'lane_join', 'lane_join_span_15'} and one(16 * 32) >= {'lane_join', 'lane_join_span_15'}
    assert one(16 * 32 + 1) >= {'wg_join', 'wg_join_span_16', 'wg_join_slot0'}
    assert 'wg_join_unrolled' not in one(17 * 16 * 32, D=16) and 'wg_join_unrolled' in one(17 * 16 * 32 + 1, D=16)
    assert 'wg_join_unrolled' in one(17 * 4 * 32 + 1, D=64) and 'wg_join_unrolled' not in one(17 * 4 * 32 + 1, D=32)
    assert 'wg_join_even_tail' in one(32 * 32, D=16) and 'wg_join_ragged_tail' in one(33 * 32, D=16)
    assert E.join_lane_pieces(16, 4) == [4, 4, 4, 4] and E.join_lane_pieces(60, 4) == [15, 15, 15, 15] and E.join_lane_pieces(64, 4) == [16] * 4
    assert E.join_lane_pieces(18, 16) == [1, 2, 2] + [1] * 13
    for D in E.D_CLASSES:                                     # unroll_layout: all lanes one short of a turn; all lanes one turn and no tail
        c = E.classify_segments(E.unroll_layout(D), D)
        assert set(E.join_lane_pieces(15 * E.NPL(D), E.NPL(D))) == {15} and 'wg_join_lane_tail_15' in c[1] and 'wg_join_unrolled' not in c[1]
        assert set(E.join_lane_pieces(16 * E.NPL(D), E.NPL(D))) == {16} and 'wg_join_lane_no_tail' in c[3]
    assert [sorted(E.classify_layout(t)) for t in E.TINY_LAYOUTS] == [
        ['all_pooled', 'last_chunk_partial', 'one_chunk_no_join'], ['all_pooled', 'last_chunk_full', 'one_chunk_no_join'],
        ['all_pooled', 'last_chunk_partial'], ['last_chunk_full', 'not_pooled_last', 'one_chunk_no_join'], ['all_pooled', 'last_chunk_partial']]


@pytest.mark.parametrize('D', (12, 17, 33))
def test_build_layout_is_a_sorted_layout(D):
    for lengths in E.layouts(D):
        lay = E.build_layout(lengths, C=7, T=3, seed=1)
        N, S = lay['N'], lay['S']
        assert N == sum(lengths) and np.array_equal(np.sort(lay['order']), np.arange(N))
        assert N < 64 or not np.array_equal(lay['order'], np.arange(N))          # not the identity
        assert np.array_equal(lay['seg_first'][:S + 1], np.concatenate([[0], np.cumsum(lengths)])) and np.all(lay['seg_first'][S:] == N)
        same = lay['seg_id'][1:] == lay['seg_id'][:-1]
        assert np.all(lay['order'][1:][same] > lay['order'][:-1][same])           # entries of a segment ascend
        ks = lay['key'][lay['order']]
        assert np.array_equal(ks[1:] == ks[:-1], same)                            # one key per segment, no key twice
        pooled = lay['seg_keys'][:-1] if E.not_pooled_last(lengths) else lay['seg_keys']
        assert np.all(np.diff(pooled) > 0) and np.all(pooled >= 0)
        if E.not_pooled_last(lengths):
            last = lay['order'][lay['first'][S - 1]:]
            assert np.all(lay['t'][last] == -1) and np.all(lay['key'][last] == E.KEY_NOT_POOLED)
            assert np.count_nonzero(lay['t'] < 0) == lengths[-1]
        else:
            assert np.all(lay['t'] >= 0)
        assert lay['t'].max() < 3 and lay['B'] * 7 >= N > (lay['B'] - 1) * 7


@pytest.mark.parametrize('D', (12, 17, 33))
@pytest.mark.parametrize('family', ('exact', 'float'))
def test_oracle_agrees_with_the_dense_formulation(D, family):
    for C in (1, 7):
        for lengths in E.layouts(D):
            lay = E.build_layout(lengths, C=C, T=3, seed=2)
            dout, w, cnt = E.bwd_values(lay, D, family, True, True)
            a = O.rows_bwd(lay['key'], lay['t'], w, cnt, dout, C, True)
            b = O.rows_bwd_dense(lay['key'], lay['t'], w, cnt, dout, C, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            if family == 'exact':
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
            else:
                assert np.all(np.abs(a[1] - b[1]) <= 1e-12 * (b[3] + 1e-300)) and np.all(np.abs(a[3] - b[3]) <= 1e-12 * (b[3] + 1e-300))
            # per key: the not-pooled key is there, with no terms; every other key counts the entries of its segment
            pos = np.searchsorted(a[0], lay['seg_keys'])
            want_n = np.where(lay['seg_keys'] == E.KEY_NOT_POOLED, 0, lay['lengths'])
            assert np.array_equal(a[0][pos], lay['seg_keys']) and np.array_equal(a[2][pos], want_n)


def test_direct_oracle_agrees_with_a_loop():
    D, V, C = 5, 64, 3
    lengths = [7, 25, 40, 3]
    for w_div in (1, 4):
        keys = np.array([-2, 5, 9, V], np.int64)
        lay = E.build_layout(lengths, C=C, T=1, seed=3, pooled_last=True, keys=keys)
        rng = np.random.default_rng(w_div)
        dout = rng.standard_normal((lay['B'], D)).astype(np.float32)
        w = rng.uniform(-1.5, 1.5, -(-lay['N'] // w_div)).astype(np.float32)
        dt, n, sabs, named = O.rows_bwd_direct(lay['key'], w, w_div, dout, C, V)
        ref = np.zeros((V, D))
        for e in range(lay['N']):
            if 0 <= lay['key'][e] < V:
                ref[lay['key'][e]] += np.float64(w[e // w_div]) * dout[e // C].astype(np.float64)
        assert np.allclose(dt, ref, rtol=1e-13, atol=0) and list(np.flatnonzero(named)) == [5, 9] and list(n[[5, 9]]) == [25, 40]


@pytest.mark.parametrize('D', E.D_CLASSES)
def test_exact_family_fits_the_fp32_window(D):
    """every term is a whole multiple of EXACT_UNIT and sum |term| stays below 2^24 units, so every partial sum of every order is an fp32 number"""
    for lengths in E.layouts(D):
        for C, mean, use_w in ((1, 1, 1), (7, 1, 1), (7, 0, 0)):
            lay = E.build_layout(lengths, C=C, T=3)
            dout, w, cnt = E.bwd_values(lay, D, 'exact', mean, use_w)
            _, sums, _, sabs = O.rows_bwd(lay['key'], lay['t'], w, cnt, dout, C, mean)
            units = sabs / E.EXACT_UNIT
            assert np.array_equal(units, np.round(units)) and np.array_equal(sums / E.EXACT_UNIT, np.round(sums / E.EXACT_UNIT))
            assert units.max() < E.EXACT_LIMIT, units.max()
            assert np.array_equal(sums.astype(np.float32).astype(np.float64), sums)
            if len(lengths) > 20:
                assert np.count_nonzero(sums) > 0.5 * sums.size                      # not a degenerate census
    # the direct route: weights only
    lengths = E.main_layout(D)
    V = 2 * len(lengths) + 8
    lay = E.build_layout(lengths, C=7, T=1, pooled_last=True, keys=E.direct_keys(lengths, D, V, True))
    rng = np.random.default_rng(D)
    dout = rng.integers(-8, 9, (lay['B'], D)).astype(np.float32)
    w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), -(-lay['N'] // 4))
    _, _, sabs, _ = O.rows_bwd_direct(lay['key'], w, 4, dout, 7, V)
    assert (sabs / E.EXACT_UNIT).max() < E.EXACT_LIMIT


def test_forward_cases_reach_every_route():
    got = set()
    for case in E.fwd_cases():
        T, D, C, B, V = case
        assert 3 <= B <= 40
        got |= E.fwd_classes(case)
    assert got == set(E.FWD_CLASSES), (set(E.FWD_CLASSES) - got, got - set(E.FWD_CLASSES))
    shapes = {(c[0], c[1]): E.fwd_route(c[0], c[1]) for c in E.fwd_cases()}
    assert shapes[(24, 16)] == ('v4', 4) and shapes[(96, 64)] == ('v4', 2) and shapes[(200, 64)] == ('v4', 1)
    assert shapes[(23, 16)] == ('scalar', 4) and shapes[(100, 70)] == ('scalar', 2) and shapes[(90, 130)] == ('scalar', 1)
    assert all(shapes[s] == ('scalar', 4) for s in ((70, 12), (9, 1), (3, 70), (5, 130)))
    assert shapes[(260, 64)] == (None, None)
    assert {c[1] for c in E.fwd_cases() if E.fwd_route(c[0], c[1])[0] == 'v4'} == {4, 8, 16, 32, 64}


def test_forward_exact_family_fits_the_fp32_window():
    for case in E.fwd_cases():
        if E.fwd_route(case[0], case[1])[0] is None:
            continue
        seg, rows, w, table = E.fwd_inputs(case, 'exact', True)
        assert (rows < 0).any() and (rows >= case[4]).any() and (seg < 0).any()
        out, cnt, n, sabs = O.pool_fwd(table, rows, seg, w, case[0], 0)
        assert sabs.max() * 2 < E.EXACT_LIMIT and np.array_equal(sabs * 2, np.round(sabs * 2))         # terms are multiples of 1/2
        assert np.array_equal(cnt, n) and np.count_nonzero(out) > 0.5 * np.count_nonzero(cnt) * case[1]

"""The sort route of the in-batch GAUC and the plain in-batch AUC (rec_block/auc.py route='sort' / in_batch_auc, csrc/pairwise_auc_sort.hip,
recnow_pair_auc_sorted_terms) against the integer oracles tests/_auc_oracle.py (quadratic) and tests/_auc_sort_oracle.py (searchsorted; pinned
to the former on the CPU in tests/test_auc_sort_cpu.py), and against the walk route bit for bit.

Bounds.  Every per-row and per-list count exact; the metric within the bounds of tests/test_pair_auc_gpu.py (1e-6 relative on the float32
ratio, 1e-12 on the fp64 sums); every output of the sort route `torch.equal` to the walk route's -- same integers, same sum kernels.

Tiles.  T = RECNOW_AUC_SORT_TILE positions of the (list, score) order go to one workgroup of the prefix-count kernels.  The `tiles` layout is
built from T and `_tiles_census` asserts in numpy, from the layout alone, what it holds (list and tie-run positions against the tile
boundaries)."""
import os

import numpy as np
import pytest
import torch

import _auc_oracle as A
import _auc_sort_oracle as S
import _pair_lists_oracle as O

pytestmark = pytest.mark.gpu

NAMES = tuple(O.LAYOUTS)
EINVAL, EWORKSPACE = -1, -2
NAN, INF = float('nan'), float('inf')
ROW_FIELDS = (('row_pairs', 'row_n'), ('row_concordant', 'row_c'), ('row_tied', 'row_t'))
LIST_FIELDS = (('list_pairs', 'N'), ('list_concordant', 'C'), ('list_tied', 'T'), ('list_rows', 'R'))


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _auc():
    from rec_now_amd.rec_block import auc
    return auc


def _T():
    return _auc().AUC_SORT_TILE


def _t(a):
    return torch.from_numpy(np.array(a))


def _dv(a, dev):
    if a is None:
        return None
    if isinstance(a, list):
        return [_t(x).to(dev) for x in a]
    return _t(a).to(dev)


_REF = {}


def _ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _lists_of_segments(seg, cnt):
    """for every segment of the library the oracle's list it is (the same rows); every list appears once"""
    B = seg.B
    order = seg.order.cpu().numpy()
    sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), B)
    n_seg = sf.size - 1
    assert n_seg == len(cnt.lists) == seg.num_segments()
    lid = cnt.list_id[order[sf[:-1]]]
    assert np.unique(lid).size == n_seg
    assert np.array_equal(np.sort(cnt.list_id[order]), np.sort(cnt.list_id)) and np.array_equal(cnt.list_id[order], np.repeat(lid, np.diff(sf)))
    return lid


def _check_terms(got, ref, lid, what):
    for field, name in ROW_FIELDS:
        have = getattr(got, field)
        assert have.dtype == torch.int32 and have.shape == (ref.row_n.size,)
        diff = np.flatnonzero(have.cpu().numpy().astype(np.int64) != getattr(ref, name))
        assert diff.size == 0, '%s %s: %d rows differ, first %s' % (what, field, diff.size, diff[:8])
    for field, name in LIST_FIELDS:
        have = getattr(got, field)
        assert have.dtype == torch.int64 and have.shape == (ref.row_n.size,)
        diff = np.flatnonzero(have.cpu().numpy()[:lid.size] != getattr(ref, name)[lid])
        assert diff.size == 0, '%s %s: %d segments differ, first %s' % (what, field, diff.size, diff[:8])


def _check_metric(got, want, what):
    assert (got.auc.dtype, got.n_lists.dtype, got.weighted_sum.dtype, got.weight_sum.dtype) == (torch.float32, torch.int64, torch.float64,
                                                                                                torch.float64)
    assert got.auc.shape == got.n_lists.shape == got.weighted_sum.shape == got.weight_sum.shape == ()
    auc, n, num, den = got.auc.item(), got.n_lists.item(), got.weighted_sum.item(), got.weight_sum.item()
    print('AUC %s: %.9g (ref %.9g) over %d lists (ref %d); sums %.17g / %.17g (ref %.17g / %.17g)'
          % (what, auc, want.auc, n, want.n_lists, num, den, want.weighted_sum, want.weight_sum))
    assert n == want.n_lists
    assert abs(auc - want.auc) <= 1e-6 * abs(want.auc)
    assert abs(num - want.weighted_sum) <= 1e-12 * abs(want.weighted_sum)
    assert abs(den - want.weight_sum) <= 1e-12 * abs(want.weight_sum)


def _same_terms(a, b, n_seg, what):
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        if f.startswith('list_'):
            x, y = x[:n_seg], y[:n_seg]                  # (the entries behind the segments are not written)
        assert x.dtype == y.dtype and torch.equal(x, y), '%s: %s of the two routes differ' % (what, f)


def _same_metric(a, b, what):
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and torch.equal(x, y), '%s: %s of the two routes differ (%r, %r)' % (what, f, x.item(), y.item())


def _both_routes(dev, s, y, groups, mask, th, ref, what, seg=None):
    """counts exact on the sort route, the metric in bounds for each weight, every output equal to the walk's"""
    M, AUC = _mod(), _auc()
    sd, yd, md, gd = _dv(s, dev), _dv(y, dev), _dv(mask, dev), _dv(groups, dev)
    seg = seg if seg is not None else M.group_rows(gd)
    lid = _lists_of_segments(seg, ref)
    got = AUC.auc_terms(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='sort')
    _check_terms(got, ref, lid, what)
    _same_terms(got, AUC.auc_terms(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='walk'), lid.size, what)
    for w in A.WEIGHTS:
        res = AUC.in_batch_gauc(sd, yd, gd, mask=md, pos_neg_th=th, weight=w, segments=None if w == 'rows' else seg, route='sort')
        _check_metric(res, A.metric(ref, w), what + ' ' + w)
        _same_metric(res, AUC.in_batch_gauc(sd, yd, None, mask=md, pos_neg_th=th, weight=w, segments=seg, route='walk'), what + ' ' + w)
    return got


# ---- 1. the three route layouts of the walk --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['one', 'two'])
@pytest.mark.parametrize('th', [None, 0.5, 1.5], ids=['graded', 'th0.5', 'th1.5'])
@pytest.mark.parametrize('use_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('name', NAMES)
def test_layouts_exact_and_equal_to_the_walk(dev, name, use_mask, th, variant):
    g, s, y, mask = O.layout(name)
    groups = [g, O.second_groups(g.size)] if variant == 'two' else g
    m = mask if use_mask else None
    ref = _ref((name, variant, use_mask, th), lambda: A.counts(s, y, groups, m, th))
    assert (ref.N == 0).any() and (ref.T > 0).any()
    _both_routes(dev, s, y, groups, m, th, ref, '%s %s %s %s' % (name, 'mask' if use_mask else 'nomask', th, variant))


# ---- 2. the tiles layout ---------------------------------------------------------------------------------------------------------------------
def _tiles_layout():
    """(list ids int32, scores, labels, mask), rows shuffled; list sizes in id order below; scores rounded so ties abound.  List 1 is the long
    one: T - 224 negative scores (two of them -inf), T + 376 zeros of both signs, T + 76 positive ones (two +inf, three NaN)."""
    def build():
        T = _T()
        rng = np.random.default_rng(97)
        sizes = [T, 3 * T + 228, 1, 1, 40, 50, 100, 7, 300, 2 * T - 48, T + 353]
        lid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
        B = lid.size
        s = (np.round(rng.normal(size=B) * 16) / 16).astype(np.float32)
        y = rng.integers(0, 4, B).astype(np.float32)
        mask = rng.random(B) < 0.85
        a = T                                                                   # list 1 begins here
        neg, zero = T - 224, T + 376
        s[a:a + neg] = -np.abs(s[a:a + neg]) - 0.0625
        s[a:a + 2] = -INF
        s[a + neg:a + neg + zero:2], s[a + neg + 1:a + neg + zero:2] = 0.0, -0.0
        pos = slice(a + neg + zero, a + sizes[1])
        s[pos] = np.abs(s[pos]) + 0.0625
        s[a + neg + zero:a + neg + zero + 2] = INF
        s[a + neg + zero + 2:a + neg + zero + 5] = NAN
        y[a + neg + zero + 1:a + neg + zero + 4] = [3.0, 3.0, 0.0]             # NaN and inf scores on the higher and on the lower side
        mask[a:a + 2] = mask[a + neg:a + neg + 4] = mask[a + neg + zero:a + neg + zero + 5] = True
        first = np.cumsum([0] + sizes)
        mask[first[4]:first[5]] = False                                         # list 4: every row masked out
        y[first[5]:first[6]] = 2.0                                              # list 5: one class
        mask[first[5]:first[5] + 2] = True
        y[a + 7], y[first[9] + 5], y[first[8] + 1] = NAN, NAN, NAN
        mask[a + 7] = mask[first[9] + 5] = mask[first[8] + 1] = True
        perm = rng.permutation(B)
        out = tuple(v[perm] for v in (lid, s, y, mask))
        for v in out:
            v.setflags(write=False)
        return out
    return _ref('tiles-layout', build)


def _tiles_census(lid, s, y, mask):
    """{property: count} of the (list, canonical score key) order against the tile boundaries; numpy on the layout alone"""
    T, B = _T(), lid.size
    order, l, k, run = S.sorted_layout(lid, s)
    n_list = int(lid.max()) + 1
    first = np.searchsorted(l, np.arange(n_list), side='left')
    end = np.searchsorted(l, np.arange(n_list), side='right')
    rfirst = np.searchsorted(run, np.arange(run[-1] + 1), side='left')
    rend = np.searchsorted(run, np.arange(run[-1] + 1), side='right')
    tile_lo, tile_hi = (rfirst + T - 1) // T, rend // T                    # whole tiles inside the run: [tile_lo, tile_hi)
    long_l = int(np.argmax(end - first))
    rows = order[first[long_l]:end[long_l]]
    take_lists = [mask[order[first[g]:end[g]]] for g in range(n_list)]
    return {
        'list_starts_on_boundary': int(((first > 0) & (first % T == 0)).sum()),
        'list_ends_on_boundary': int(((end < B) & (end % T == 0)).sum()),
        'tile_with_3_lists': int(sum(np.unique(l[t:t + T]).size >= 3 for t in range(0, B, T))),
        'list_over_3_tiles': int((((end - 1) // T - first // T + 1) >= 3).sum()),
        'run_crossing_boundary': int((((rend - 1) // T) > (rfirst // T)).sum()),
        'run_over_a_whole_tile_and_both_sides': int(((tile_hi > tile_lo) & (rfirst < tile_lo * T) & (rend > tile_hi * T)).sum()),
        'one_row_lists': int((end - first == 1).sum()),
        'all_masked_lists': int(sum(1 for m in take_lists if m.size > 1 and not m.any())),
        'single_class_lists': int(sum(1 for g in range(n_list) if take_lists[g].sum() >= 2
                                      and np.unique(y[order[first[g]:end[g]]][take_lists[g]]).size == 1)),
        'long_list_nan_scores': int((np.isnan(s[rows]) & mask[rows]).sum()),
        'long_list_infs': int(np.isposinf(s[rows]).any()) + int(np.isneginf(s[rows]).any()),
        'long_list_zeros': int(((s[rows] == 0) & np.signbit(s[rows])).any()) + int(((s[rows] == 0) & ~np.signbit(s[rows])).any()),
        'long_list_tiles': int((end[long_l] - 1) // T - first[long_l] // T + 1),
        'nan_labels_taking_part': int((np.isnan(y) & mask).sum()),
        'partial_last_tile': int(B % T != 0),
    }


def test_tiles_layout_holds_what_it_is_for():
    c = _tiles_census(*_tiles_layout())
    print('tiles census: %s' % c)
    assert _tiles_layout()[0].size == 7 * _T() + 1032
    for key in ('list_starts_on_boundary', 'list_ends_on_boundary', 'tile_with_3_lists', 'list_over_3_tiles', 'run_crossing_boundary',
                'run_over_a_whole_tile_and_both_sides', 'all_masked_lists', 'single_class_lists', 'nan_labels_taking_part', 'partial_last_tile'):
        assert c[key] >= 1, key
    assert c['one_row_lists'] >= 2 and c['long_list_nan_scores'] >= 2 and c['long_list_infs'] == 2 and c['long_list_zeros'] == 2
    assert c['long_list_tiles'] >= 3


@pytest.mark.parametrize('th', [None, 1.5], ids=['graded', 'th1.5'])
@pytest.mark.parametrize('use_mask', [True, False], ids=['mask', 'nomask'])
def test_tiles_layout_exact_and_equal_to_the_walk(dev, use_mask, th):
    lid, s, y, mask = _tiles_layout()
    m = mask if use_mask else None
    ref = _ref(('tiles', use_mask, th), lambda: A.counts(s, y, lid, m, th))
    assert (ref.N == 0).any() and (ref.T > 0).any() and ref.row_n[np.isnan(s)].sum() > 0
    _both_routes(dev, s, y, lid, m, th, ref, 'tiles %s %s' % ('mask' if use_mask else 'nomask', th))


# ---- 3. the grouping routes of the inner sort -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,big', [(5000, 700), (300000, 20000), (1200000, 50000)], ids=['B5000', 'B300000', 'B1200000'])
def test_inner_sort_routes(dev, B, big):
    """two key words: the cooperative launch at 2048 keys per workgroup, at 4096 (from 262 144 rows on), and the multi-launch chain (above
    1 048 576 rows).  One list of `big` rows, the rest lists of 64 rows or fewer; int32 ids, so list k is segment k."""
    M, AUC = _mod(), _auc()
    rng = np.random.default_rng(B)
    n_small = (B - big + 63) // 64
    sizes = np.concatenate([[big], np.full(n_small, 64)])
    sizes[-1] -= sizes.sum() - B
    lid = np.repeat(np.arange(sizes.size), sizes).astype(np.int32)
    rng.shuffle(lid)
    s = (np.round(rng.normal(size=B) * 64) / 64).astype(np.float32)
    s[rng.integers(0, B, 50)] = NAN
    y = rng.integers(0, 4, B).astype(np.float32)
    mask = rng.random(B) < 0.9
    sd, yd, md, gd = _dv(s, dev), _dv(y, dev), _dv(mask, dev), _dv(lid, dev)
    seg = M.group_rows(gd)
    assert np.array_equal(np.diff(O.trim_seg_first(seg.seg_first.cpu().numpy(), B)), sizes)
    for th in (None, 1.5):
        ref = S.counts(s, y, lid, mask, th)
        assert ref.T.sum() > 0 and ref.N[0] > 0 and ref.row_n[np.isnan(s)].sum() > 0
        got = AUC.auc_terms(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='sort')
        _check_terms(got, ref, np.arange(sizes.size), 'B=%d th=%s' % (B, th))
        _same_terms(got, AUC.auc_terms(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='walk'), sizes.size, 'B=%d th=%s' % (B, th))
        res = AUC.in_batch_gauc(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='sort')
        _check_metric(res, A.metric(ref, 'rows'), 'B=%d th=%s' % (B, th))
        _same_metric(res, AUC.in_batch_gauc(sd, yd, None, mask=md, pos_neg_th=th, segments=seg, route='walk'), 'B=%d th=%s' % (B, th))


# ---- 4. in_batch_auc ---------------------------------------------------------------------------------------------------------------------------
def _metric_tuple(res):
    return res.auc.item(), res.n_lists.item(), res.weighted_sum.item(), res.weight_sum.item()


@pytest.mark.parametrize('route', ['walk', 'sort', 'auto'])
def test_in_batch_auc_tiny_batches(dev, route):
    AUC = _auc()
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)      # noqa: E731
    for s, y in (([], []), ([0.3], [1.0]), ([0.3, 0.3], [1.0, 1.0])):
        assert _metric_tuple(AUC.in_batch_auc(f(s), f(y), route=route)) == (0.0, 0, 0.0, 0.0)
        terms = AUC.auc_batch_terms(f(s), f(y), route=route)
        assert all(t.shape == (len(s),) for t in terms) and not any(t[:1].any().item() for t in terms[:6])
        assert len(s) == 0 or terms.list_rows[0].item() == len(s)
    assert _metric_tuple(AUC.in_batch_auc(f([2.0, 1.0]), f([1.0, 0.0]), route=route)) == (1.0, 1, 1.0, 1.0)
    assert _metric_tuple(AUC.in_batch_auc(f([1.0, 2.0]), f([1.0, 0.0]), route=route)) == (0.0, 1, 0.0, 1.0)
    # five rows by hand: positives 0 (0.9) and 3 (0.5), negatives 1 (0.9: tie with row 0), 2 (0.1: below both) and 4 (NaN: discordant twice)
    s, y = f([0.9, 0.9, 0.1, 0.5, NAN]), f([1, 0, 0, 1, 0])
    res = AUC.in_batch_auc(s, y, route=route)
    assert _metric_tuple(res) == (np.float32(2.5 / 6.0), 1, 2.5, 6.0)
    terms = AUC.auc_batch_terms(s.reshape(5, 1), y.reshape(5, 1), route=route)
    assert terms.row_pairs.tolist() == [3, 0, 0, 3, 0] and terms.row_concordant.tolist() == [1, 0, 0, 1, 0]
    assert terms.row_tied.tolist() == [1, 0, 0, 0, 0]
    assert [t[0].item() for t in terms[3:]] == [6, 2, 1, 5]
    res = AUC.in_batch_auc(s, y, mask=f([1, 0, 1, 1, 1]), pos_neg_th=0.5, route=route)      # without row 1: N = 4, C = 2, T = 0
    assert _metric_tuple(res) == (0.5, 1, 2.0, 4.0)


@pytest.mark.parametrize('th', [None, 0.5], ids=['graded', 'th0.5'])
def test_in_batch_auc_against_the_oracle(dev, th):
    AUC = _auc()
    B = 3 * _T() + 5
    rng = np.random.default_rng(12)
    s = (np.round(rng.normal(size=B) * 32) / 32).astype(np.float32)
    s[[5, B // 2]] = NAN
    y = rng.integers(0, 3, B).astype(np.float32)
    mask = rng.random(B) < 0.9
    ref = _ref(('one-list', th), lambda: A.counts(s, y, np.zeros(B, dtype=np.float32), mask, th))
    assert ref.T[0] > 0 and ref.C[0] > 0
    sd, yd, md = _dv(s, dev), _dv(y, dev), _dv(mask, dev)
    res = {r: AUC.in_batch_auc(sd, yd, mask=md, pos_neg_th=th, route=r) for r in ('walk', 'sort')}
    terms = {r: AUC.auc_batch_terms(sd, yd, mask=md, pos_neg_th=th, route=r) for r in ('walk', 'sort')}
    for r in ('walk', 'sort'):
        _check_metric(res[r], A.metric(ref, 'pairs'), 'one list %s %s' % (r, th))
        assert res[r].weighted_sum.item() == (2 * int(ref.C[0]) + int(ref.T[0])) / 2.0 and res[r].weight_sum.item() == float(ref.N[0])
        _check_terms(terms[r], ref, np.zeros(1, dtype=np.int64), 'one list %s %s' % (r, th))
    _same_metric(res['walk'], res['sort'], 'one list')
    _same_terms(terms['walk'], terms['sort'], 1, 'one list')
    # the same batch through in_batch_gauc with a constant group tensor
    g0 = torch.zeros(B, device=dev)
    _same_metric(res['sort'], AUC.in_batch_gauc(sd, yd, g0, mask=md, pos_neg_th=th, weight='pairs', route='sort'), 'constant group')


def test_in_batch_auc_auto_takes_the_route_by_size(dev, monkeypatch):
    AUC = _auc()
    from rec_now_amd import _lib
    monkeypatch.setattr(AUC, 'AUC_SORT_FROM', 64)
    called, real = [], _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (called.append(name), real(name, *a))[1])
    for B in (63, 64):
        z = torch.zeros(B, device=dev)
        AUC.in_batch_auc(z, z)
    assert called == ['recnow_pair_auc_terms', 'recnow_pair_auc_sorted_terms']         # and no grouping call in front of either


@pytest.mark.parametrize('route', ['walk', 'sort'])
def test_in_batch_auc_exact_values(dev, route):
    AUC = _auc()
    rng = np.random.default_rng(3)
    B = 2 * _T() + 77
    y = rng.integers(0, 4, B).astype(np.float32)
    res = AUC.in_batch_auc(torch.full((B,), 0.25, device=dev), _dv(y, dev), route=route)
    N = int((np.bincount(y.astype(np.int64), minlength=4)[:, None] * np.bincount(y.astype(np.int64), minlength=4)[None, :])[np.tril_indices(4, -1)].sum())
    assert _metric_tuple(res) == (0.5, 1, N / 2.0, float(N))
    for th in (None, 1.5):
        for sign, want in ((1.0, 1.0), (-1.0, 0.0)):
            s = (sign * (y + 0.125)).astype(np.float32)
            res = AUC.in_batch_auc(_dv(s, dev), _dv(y, dev), pos_neg_th=th, route=route)
            assert res.auc.item() == want and res.n_lists.item() == 1 and res.weighted_sum.item() == want * res.weight_sum.item()


# ---- 5. classes -------------------------------------------------------------------------------------------------------------------------------
VALUES_16 = [-INF, -2.5, -1.0, -2.0 ** -20, 0.0, 2.0 ** -20, 0.5, 1.0, 1.5, 2.0, 3.0, 7.0, 100.0, 1e30, 3e38, INF]


def _class_batch(values, B=3000, seed=21):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 5, B).astype(np.float32)
    y = np.array(values, dtype=np.float32)[rng.integers(0, len(values), B)]
    y[:len(values)] = values                                       # every value occurs
    y[y == 0] = np.where(rng.random(int((y == 0).sum())) < 0.5, -0.0, 0.0).astype(np.float32)      # both zeros: one value
    s = (np.round(rng.normal(size=B) * 8) / 8).astype(np.float32)
    mask = rng.random(B) < 0.9
    mask[:len(values)] = True
    return g, s, y, mask


def _is_poisoned(terms, res, B):
    ok = all(t.shape == (B,) and bool((t == -1).all().item()) for t in terms)
    return ok and res.n_lists.item() == -1 and all(np.isnan(v.item()) for v in (res.auc, res.weighted_sum, res.weight_sum))


def test_sixteen_label_values_are_exact(dev):
    g, s, y, mask = _class_batch(VALUES_16)
    assert np.unique(y[mask]).size == 16 and np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    y = y.copy()
    y[20:24] = NAN                                                 # NaN labels are no value
    _both_routes(dev, s, y, g, mask, None, A.counts(s, y, g, mask), '16 values')


def test_seventeen_label_values_poison_the_call(dev):
    AUC = _auc()
    g, s, y, mask = _class_batch(VALUES_16 + [5.0])
    assert np.unique(y[mask]).size == 17
    sd, yd, md, gd = (_dv(a, dev) for a in (s, y, mask, g))
    terms = AUC.auc_terms(sd, yd, gd, mask=md, route='sort')
    res = AUC.in_batch_gauc(sd, yd, gd, mask=md, route='sort')
    assert _is_poisoned(terms, res, g.size)
    assert AUC.in_batch_auc(sd, yd, mask=md, route='sort').n_lists.item() == -1
    # the binary rule has two classes whatever the labels, and the walk knows no classes
    ref = A.counts(s, y, g, mask, 1.25)
    _both_routes(dev, s, y, g, mask, 1.25, ref, '17 values, binary rule')
    assert AUC.in_batch_gauc(sd, yd, gd, mask=md, route='walk').n_lists.item() == 5


def test_seventeenth_value_on_masked_rows_only_is_exact(dev):
    g, s, y, mask = _class_batch(VALUES_16 + [5.0])
    mask = mask & (y != 5.0)
    assert np.unique(y).size == 17 and np.unique(y[mask]).size == 16
    _both_routes(dev, s, y, g, mask, None, A.counts(s, y, g, mask), '17th value masked out')


def test_continuous_labels_under_the_binary_rule(dev):
    rng = np.random.default_rng(22)
    B = 4000
    g = rng.integers(0, 7, B).astype(np.float32)
    y = rng.random(B).astype(np.float32)
    y[:3] = [NAN, 0.5, INF]
    s = (np.round(rng.normal(size=B) * 8) / 8).astype(np.float32)
    assert np.unique(y[~np.isnan(y)]).size > 1000
    _both_routes(dev, s, y, g, None, 0.5, A.counts(s, y, g, None, 0.5), 'continuous labels')


# ---- 6. the C entry ----------------------------------------------------------------------------------------------------------------------------
def _c_call(dev, seg, sd, yd, m8, flags, binary, th, weight, ws, nbytes=None, entry='recnow_pair_auc_sorted_terms'):
    """every output of the entry, as host arrays, from buffers filled with -7 / NaN beforehand; the return code first"""
    from rec_now_amd import _lib
    B, P = seg.B, _lib.ptr
    rows = [torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    lists = [torch.full((max(B, 1),), -7, dtype=torch.int64, device=dev) for _ in range(4)]
    auc = torch.full((1,), NAN, dtype=torch.float32, device=dev)
    num, den = (torch.full((1,), NAN, dtype=torch.float64, device=dev) for _ in range(2))
    n_lists = torch.full((1,), -7, dtype=torch.int64, device=dev)
    outs = rows + lists + [auc, num, den, n_lists]
    rc = getattr(_lib.load(), entry)(P(sd), P(yd), P(m8), P(seg.order), P(seg.seg_id), P(seg.seg_first), B, flags, binary, th, weight,
                                     *[P(t) for t in outs], P(ws), ws.numel() if nbytes is None else nbytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize('th', [None, 0.5], ids=['graded', 'th0.5'])
def test_c_entry_run_to_run_and_against_the_walk_entry(dev, th):
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, mask = O.layout('chain')
    seg = M.group_rows(_t(g).to(dev))
    sd, yd, m8 = _t(s).to(dev), _t(y).to(dev), _t(mask).to(dev).to(torch.uint8).contiguous()
    lib = _lib.load()
    nbytes = lib.recnow_pair_auc_sorted_workspace_bytes(seg.B)
    args = (0, 0 if th is None else 1, th or 0.0, 0)
    runs = [_c_call(dev, seg, sd, yd, m8, *args, _lib.workspace(nbytes, dev)) for _ in range(2)]
    walk = _c_call(dev, seg, sd, yd, m8, *args, _lib.workspace(lib.recnow_pair_auc_workspace_bytes(seg.B), dev), entry='recnow_pair_auc_terms')
    assert runs[0][0] == runs[1][0] == walk[0] == 0
    for a, b, c in zip(runs[0][1], runs[1][1], walk[1]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert runs[0][1][0].max() > 0 and runs[0][1][10][0] > 0 and 0.0 < runs[0][1][7][0] < 1.0
    # one byte short
    rc, outs = _c_call(dev, seg, sd, yd, m8, *args, _lib.workspace(nbytes, dev), nbytes=nbytes - 1)
    assert rc == EWORKSPACE and outs[10][0] == -7


def test_c_entry_refuses_bad_arguments(dev):
    """return codes only: every refusal comes before the first launch"""
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, _ = O.layout('r2049')
    seg = M.group_rows(_t(g).to(dev))
    sd, yd = _t(s).to(dev), _t(y).to(dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.recnow_pair_auc_sorted_workspace_bytes(seg.B), dev)

    def rc(flags=0, binary=0, th=0.0, weight=0, nbytes=None, sd=sd):
        return _c_call(dev, seg, sd, yd, None, flags, binary, th, weight, ws, nbytes)[0]
    assert rc() == 0
    assert rc(weight=3) == EINVAL and rc(weight=-1) == EINVAL
    assert rc(flags=1) == EINVAL and rc(flags=256 | 2) == EINVAL
    assert rc(flags=256) == EINVAL                                                 # RECNOW_PAIR_MEMBERS_PACKED: refused on this route
    assert rc(binary=1, th=NAN) == EINVAL and rc(binary=1, th=INF) == EINVAL
    assert rc(nbytes=lib.recnow_pair_auc_workspace_bytes(seg.B)) == EWORKSPACE
    assert rc(sd=None) == EINVAL
    assert lib.recnow_pair_auc_sorted_terms(None, None, None, None, None, None, seg.B, 0, 0, 0.0, 0, *([None] * 11), _lib.ptr(ws), ws.numel(),
                                            _lib.stream()) == EINVAL               # NULL segment arrays with B > 0
    assert lib.recnow_pair_auc_sorted_workspace_bytes(-1) == 0
    zd = torch.zeros(0, device=dev)
    rc0, outs = _c_call(dev, M.group_rows(zd), zd, zd, None, 0, 0, 0.0, 0, _lib.workspace(16, dev))
    assert rc0 == 0 and [float(o[0]) for o in outs[7:]] == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize('dtype', [torch.int64, torch.float64], ids=['int64', 'float64'])
def test_id_dtypes_and_column_inputs(dev, dtype):
    """an int64 / float64 id tensor whose values a float32 would merge, and outputs, labels and mask of shape (B, 1)"""
    rng = np.random.default_rng(8)
    B = 300
    small = rng.integers(0, 5, B)
    ids = (2 ** 40 + small) if dtype == torch.int64 else (1.0 + small * 2.0 ** -40)
    s = (np.round(rng.normal(size=B) * 4) / 4).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    mask = rng.random(B) < 0.9
    ref = A.counts(s, y, small, mask)
    assert len(ref.lists) == 5 and (ref.N > 0).all() and ref.T.sum() > 0
    AUC = _auc()
    gd = torch.from_numpy(np.asarray(ids)).to(dtype).to(dev)
    sd, yd, md = (_t(a).to(dev).reshape(B, 1) for a in (s, y, mask))
    terms = AUC.auc_terms(sd, yd, gd, mask=md, route='sort')
    seg = _mod().group_rows(gd)
    _check_terms(terms, ref, _lists_of_segments(seg, ref), str(dtype))
    _check_metric(AUC.in_batch_gauc(sd, yd, gd.reshape(B, 1), mask=md, weight='uniform', route='sort'), A.metric(ref, 'uniform'), str(dtype))


# ---- 7. a grouping time-out ----------------------------------------------------------------------------------------------------------------------
def test_grouping_timeout_poisons_the_sort_route(dev):
    """RECNOW_DEBUG_GROUP_TIMEOUT=1 makes every barrier of the cooperative grouping launch report a time-out at once (own process: the switch
    is read once).  The inner sort then leaves the identity order and n_seg = -1; the sort route stays in bounds on it and poisons its outputs."""
    import subprocess
    import sys
    code = r'''
import numpy as np, torch
from rec_now_amd.rec_block import auc
from rec_now_amd.rec_block._segments import Segments
dev = torch.device('cuda:0')
rng = np.random.default_rng(0)
B = 20000
y = torch.from_numpy(rng.integers(0, 3, B).astype(np.float32)).to(dev)
s = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev)
# segments that are a real grouping (built by hand: the grouping call of this process would time out as well): 20 lists of 1000 rows
seg = Segments()
seg.B, seg.device = B, dev
seg.order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
seg.seg_id = (torch.arange(B, device=dev) // 1000).to(torch.int32)
seg.seg_first = torch.full((B + 1,), B, dtype=torch.int32, device=dev)
seg.seg_first[:20] = torch.arange(0, B, 1000, dtype=torch.int32, device=dev)
seg.super_id, seg.n_seg = seg.seg_id, torch.tensor([20, 20], dtype=torch.int32, device=dev)
for th in (None, 0.5):
    terms = auc.auc_terms(s, y, None, pos_neg_th=th, segments=seg, route='sort')
    res = auc.in_batch_gauc(s, y, None, pos_neg_th=th, segments=seg, route='sort')
    torch.cuda.synchronize()
    assert all(t.shape == (B,) and bool((t == -1).all().item()) for t in terms), [t[:4] for t in terms]
    assert res.n_lists.item() == -1 and all(np.isnan(v.item()) for v in (res.auc, res.weighted_sum, res.weight_sum)), res
    walk = auc.in_batch_gauc(s, y, None, pos_neg_th=th, segments=seg, route='walk')          # the walk calls no grouping: untouched
    assert walk.n_lists.item() == 20 and 0.0 < walk.auc.item() < 1.0
one = auc.in_batch_auc(s, y, route='sort')
assert one.n_lists.item() == -1 and np.isnan(one.auc.item())
print('poisoned ok')
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=root,
                         env=dict(os.environ, RECNOW_DEBUG_GROUP_TIMEOUT='1', PYTHONPATH=root))
    assert out.returncode == 0 and 'poisoned ok' in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]

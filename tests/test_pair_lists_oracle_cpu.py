"""CPU: the per-list fp64 oracle of the pairwise loss (tests/_pair_lists_oracle.py) pinned against the dense oracles -- tests/_lambda_oracle.py
for every loss, rule and option, oracle/dense_ref.py for plain BPR -- within 1e-12 relative on seeded small batches, its per-list and per-row
outputs checked against each other, and the layouts of the route tests held to the census classes they are built for (no kernel runs here)."""
import itertools

import numpy as np
import pytest
import torch

import dense_ref as R
import _lambda_oracle as D
import _pair_lists_oracle as O

RTOL = 1e-12


def _t(a):
    return torch.from_numpy(np.array(a))


_SMALL = {}


def _small(name):
    """'one': 193 rows in 6 lists; 'two': 157 rows, 4 main groups split by a second tensor of 3 values (the occurrence count then spans lists)"""
    if name not in _SMALL:
        rng = np.random.default_rng({'one': 5, 'two': 6}[name])
        B, G = {'one': (193, 6), 'two': (157, 4)}[name]
        g = rng.integers(0, G, B).astype(np.float32)
        groups = g if name == 'one' else [g, rng.integers(0, 3, B).astype(np.float32)]
        s = (np.round(rng.normal(size=B) * 256) / 256).astype(np.float32)
        y = rng.integers(0, 4, B).astype(np.float32)
        mask = rng.random(B) < 0.8
        _SMALL[name] = (groups, s, y, mask)
    return _SMALL[name]


def _dense(groups, s, y, mask, kind, margin, factor, reduce_mean, wf, wrong, power, lam):
    s64 = _t(s).double().requires_grad_(True)
    loss, n = D.pairwise_loss(s64, y, groups, D.ref_loss(kind, margin, factor, reduce_mean), wrong, power, mask, wf, lam)
    if n:
        loss.backward()
    return loss.item(), n, (s64.grad.numpy() if s64.grad is not None else np.zeros(s.size))


def _same(got, want):
    loss, n, grad = want
    assert got.n_pair == n
    assert abs(got.loss - loss) <= RTOL * abs(loss)
    assert np.abs(got.grad - grad).max() <= RTOL * np.abs(grad).max()


@pytest.mark.parametrize('lam', [None, ('exp2', None), ('linear', 5)])
@pytest.mark.parametrize('kind', O.KINDS)
def test_oracle_is_the_dense_oracle(kind, lam):
    margin = 0.75 + O.KINK if kind == 'hinge' else 0.75
    for name, rule, wrong, power, use_mask in itertools.product(('one', 'two'), (None, O.w_sym), (False, True), (0.0, -0.5, 1.0), (True, False)):
        groups, s, y, mask = _small(name)
        m = mask if use_mask else None
        reduce_mean = power != 1.0                                                     # the raw sum on a third of the cases
        got = O.pairwise_loss(s, y, groups, kind, margin, 0.5, reduce_mean, rule, wrong, power, m, lam)
        _same(got, _dense(groups, s, y, m, kind, margin, 0.5, reduce_mean, None if rule is None else D.w_sym, wrong, power, lam))
        assert got.n_pair > 0
        # what the oracle says per list and per row adds up to what it says of the batch
        assert sum(l.n_pair for l in got.lists) == got.n_pair == int(got.cnt_row.sum())
        denom = got.n_pair + 1e-10 if reduce_mean else 1.0
        assert abs(sum(l.loss_sum for l in got.lists) / denom - got.loss) <= RTOL * abs(got.loss)
        assert sorted(np.concatenate([l.rows for l in got.lists]).tolist()) == list(range(s.size))
        for l in got.lists:
            assert int(got.cnt_row[l.rows].sum()) == l.n_pair
            if l.n_pair == 0:
                assert l.loss_sum == 0.0 and not got.grad[l.rows].any()
        if m is not None:
            assert not got.grad[~m].any() and not got.cnt_row[~m].any()


@pytest.mark.parametrize('tied', [False, True])
@pytest.mark.parametrize('name', ['one', 'two'])
def test_plain_bpr_is_the_dense_reference(name, tied):
    """oracle/dense_ref.pairwise_loss with its own bpr_loss_func.  That function writes softplus(-x) as clamp(x, 0) - x + log1p(exp(-|x|)),
    whose autograd derivative at x == 0 exactly is 0 (the subgradients torch picks for clamp and abs), not -1/2.  So its gradient is compared on
    scores without ties; on the scores of the route tests (a grid of 1/256, full of ties) its loss and count are, and the gradient of the
    same reference with the smooth softplus of tests/_lambda_oracle.py as the pair loss."""
    groups, s, y, mask = _small(name)
    if not tied:
        s = np.random.default_rng(9).normal(size=s.size).astype(np.float32)
        assert np.unique(s).size == s.size
    for wrong, power, use_mask in itertools.product((False, True), (0.0, -0.5, 1.0), (True, False)):
        gt = [_t(g) for g in groups] if isinstance(groups, list) else _t(groups)
        kw = dict(only_use_wrong_order_pair=wrong, return_num_pair=True, click_occurance_power=power, mask=_t(mask) if use_mask else None)
        got = O.pairwise_loss(s, y, groups, 'bpr', wrong=wrong, power=power, mask=mask if use_mask else None)
        s64 = _t(s).double().requires_grad_(True)
        loss, n = R.pairwise_loss(s64, _t(y).double(), gt, **kw)
        assert got.n_pair == int(n) > 0 and abs(got.loss - loss.item()) <= RTOL * abs(loss.item())
        if tied:
            s64 = _t(s).double().requires_grad_(True)
            loss, n = R.pairwise_loss(s64, _t(y).double(), gt, pairloss_func=D.ref_loss('bpr'), **kw)
        loss.backward()
        _same(got, (loss.item(), int(n), s64.grad.numpy()))


def test_rank_terms_are_the_dense_oracle():
    for name, use_mask, (gain, topn) in itertools.product(('one', 'two'), (True, False), (('exp2', None), ('linear', 5), ('exp2', 1))):
        groups, s, y, mask = _small(name)
        m = mask if use_mask else None
        a, b = O.rank_terms(s, y, groups, m, gain, topn), D.rank_terms(s, y, groups, m, gain, topn)
        assert np.array_equal(a.rank, b.rank) and np.array_equal(a.list_id, b.list_id)
        for x, z in ((a.discount, b.discount), (a.gain, b.gain), (a.inv_idcg, b.inv_idcg), (a.dcg, b.dcg), (a.idcg, b.idcg)):
            assert np.abs(x - z).max() <= RTOL * np.abs(z).max()
        assert abs(a.ndcg_mean - b.ndcg_mean) <= RTOL and a.n_lists == b.n_lists


def test_a_given_structure_changes_nothing():
    groups, s, y, mask = _small('two')
    st = O.structure(s, y, groups, O.w_sym, True, mask)
    a = O.pairwise_loss(s, y, groups, 'margin_bpr', 0.3, 2.0, True, O.w_sym, True, -0.5, mask, ('exp2', None), pairs=st)
    b = O.pairwise_loss(s, y, groups, 'margin_bpr', 0.3, 2.0, True, O.w_sym, True, -0.5, mask, ('exp2', None))
    assert a.loss == b.loss and np.array_equal(a.grad, b.grad) and np.array_equal(a.cnt_row, st.cnt_row)


def test_the_kink_check_sees_a_candidate_on_the_kink():
    g = np.zeros(4, dtype=np.float32)
    s = np.array([0.0, 1.0, 0.25, -3.0], dtype=np.float32)
    O.assert_off_the_kink(g, s, 1.0 + O.KINK, 1.0)
    with pytest.raises(AssertionError):
        O.assert_off_the_kink(g, s, 1.0, 1.0)                        # 1 - (1 - 0) = 0
    O.assert_off_the_kink(np.arange(4, dtype=np.float32), s, 1.0, 1.0)      # four lists of one row: no candidate at all


# ---- layouts and census ------------------------------------------------------------------------------------------------------------------
def _seg_first(name):
    return np.concatenate([[0], np.cumsum(O.LAYOUTS[name])])


def test_layouts_are_what_they_claim():
    for name, sizes in O.LAYOUTS.items():
        g, s, y, mask = O.layout(name)
        B = g.size
        assert B == sum(sizes) <= 7000 and B % 64 != 0
        assert np.bincount(g.astype(np.int64)).tolist() == sizes
        assert np.array_equal(s, np.round(s * 256) / 256)
        assert 0.75 < mask.mean() < 0.85
        unknown = ~np.isin(y, O.LEVELS)
        assert unknown.sum() == (1 if name == 'r2048' else 0) and not mask[unknown].any()
        assert O.layout(name)[1] is s and not s.flags.writeable


def test_census_of_a_layout_worked_by_hand():
    """sizes 600, 3, 61, 1408, 2049, 70 (B = 4191): worked out on paper from stage_members and the phase loop."""
    sf = np.concatenate([[0], np.cumsum([600, 3, 61, 1408, 2049, 70])])        # 0 600 603 664 2072 4121 4191
    # the array group_rows hands back has B + 1 entries, written up to seg_first[n_seg] == B
    c = O.census(np.concatenate([sf, np.full(4191 + 1 - sf.size, -7)]), 4191)
    # T blocks: 0, 1 all long; 2 (512..767): range [0, 2072) = 2072, not staged, 64 short rows; 3..7 inside the 1408;
    # 8 (2048..2303): range [664, 4121) not staged, no short row; 9..15 inside the 2049; 16 (4096..4190): range [2072, 4191) = 2119, 70 short rows
    assert c['t_lds'] == 0 and c['t_global'] == 64 + 70 and c['t_range_2048'] == 0 and c['t_range_2049'] == 0
    assert c['w_lds'] == 2 and c['w_global'] == 1
    assert [c['size_%d' % n] for n in (1, 2, 512, 513, 2048, 2049)] == [0, 0, 0, 0, 0, 1]
    # W blocks: 9 (576..639): (staged 600, short 61); 10 (640..703): (short 61, staged 1408); 32 (2048..2111): (staged, global);
    # 64 (4096..4159): (global, short)
    assert (c['w64_long_short'], c['w64_short_long'], c['w64_staged_global'], c['w64_global_staged'], c['w64_staged_staged']) == (2, 1, 1, 0, 0)
    assert c['long_last'] == 0 and c['long_on_64'] == 0 and c['long_on_256'] == 0
    c = O.census([0, 256, 832, 1345], 1345)                                 # 256 short; 576 long from 256; 513 long from 832 = 13 * 64, to B
    assert c['long_on_256'] == 1 and c['long_on_64'] == 1 and c['long_last'] == 1 and c['w64_staged_staged'] == 0 and c['t_lds'] == 256
    assert O.census([0, 1], 1)['size_1'] == 1 and O.census([0, 2, 77], 2)['size_2'] == 1


def test_the_layouts_reach_every_class():
    got = {name: O.census(_seg_first(name), sum(sizes)) for name, sizes in O.LAYOUTS.items()}
    for cls in O.CLASSES:
        assert any(c[cls] > 0 for c in got.values()), cls
    # and each layout what it is there for
    assert got['r2049']['t_range_2049'] == 1 and got['r2049']['t_global'] == 148 and got['r2049']['long_on_256'] == 1
    assert got['r2049']['long_on_64'] == 1
    assert got['r2048']['t_range_2048'] == 1 and got['r2048']['t_range_2049'] == 0 and got['r2048']['t_global'] == 133 + 43
    assert got['r2048']['w64_short_long'] == 1 and got['r2048']['size_512'] == 1
    c = got['chain']
    assert (c['w64_staged_global'], c['w64_global_staged'], c['w64_staged_staged'], c['w64_long_short'], c['w64_short_long']) == (1, 1, 1, 1, 1)
    assert c['long_last'] == 1 and c['size_513'] == c['size_2049'] == c['size_2048'] == c['size_512'] == c['size_2'] == c['size_1'] == 1

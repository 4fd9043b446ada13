"""Pins tests/_approx_ndcg_oracle.py, on the CPU: to a three-row list worked by hand, to torch autograd in fp64 on a dense restatement, to the
hard NDCG of tests/_pair_lists_oracle.py at a temperature at which the soft positions are the hard ones, and to the zero sum of every list's
gradient.  Also what the oracle says of the layouts the GPU tests use, and the argument errors of rec_block/approx_ndcg.py, which need no
device."""
import math

import numpy as np
import pytest
import torch

import _approx_ndcg_oracle as AO
import _pair_lists_oracle as O


def test_a_three_row_list_worked_by_hand():
    """tau = 1, scores (ln 3, 0, 0): sigma(ln 3) = 3/4, sigma(-ln 3) = 1/4, sigma(0) = 1/2, so R = (1/2, 5/4, 5/4); sigma' = 3/16 between the first
    row and the others and 1/4 between the two others.  Labels (1, 0, 2): G = (1, 0, 3), label positions (1, 2, 0)."""
    s = np.array([math.log(3.0), 0.0, 0.0])
    y = np.array([1.0, 0.0, 2.0])
    res = AO.approx_ndcg(s, y, np.zeros(3), gain='exp2', temperature=1.0)
    R = [0.5, 1.25, 1.25]
    np.testing.assert_allclose(res.approx_rank, R, rtol=1e-14)
    idcg = 3.0 / math.log2(2.0) + 1.0 / math.log2(3.0)
    adcg = 1.0 / math.log2(2.5) + 3.0 / math.log2(3.25)
    assert abs(res.idcg[0] - idcg) <= 1e-14 * idcg and abs(res.adcg[0] - adcg) <= 1e-14 * adcg
    assert res.n_lists == 1 and abs(res.loss + adcg / idcg) <= 1e-14 and -1.0 <= res.loss <= 0.0
    c = [g * math.log(2.0) / ((2.0 + r) * math.log(2.0 + r) ** 2) for g, r in zip((1.0, 0.0, 3.0), R)]
    want = [(3 / 16 * (c[1] - c[0]) + 3 / 16 * (c[2] - c[0])) / idcg,
            (3 / 16 * (c[0] - c[1]) + 1 / 4 * (c[2] - c[1])) / idcg,
            (3 / 16 * (c[0] - c[2]) + 1 / 4 * (c[1] - c[2])) / idcg]
    np.testing.assert_allclose(res.grad, want, rtol=1e-13)
    assert res.grad[2] < 0 < res.grad[1]           # raising the best row's score lowers the loss
    # linear gain: G = y
    lin = AO.approx_ndcg(s, y, np.zeros(3), gain='linear', temperature=1.0)
    assert abs(lin.idcg[0] - (2.0 + 1.0 / math.log2(3.0))) <= 1e-14 and abs(lin.adcg[0] - (1.0 / math.log2(2.5) + 2.0 / math.log2(3.25))) <= 1e-14


def _dense(s, y, lid, take, gain, tau):
    """The same loss from torch operators on (B, B) matrices, differentiable in s (fp64)."""
    same = torch.from_numpy(lid[:, None] == lid[None, :])
    t = torch.from_numpy(take)
    B = s.numel()
    ok = same & t[None, :] & t[:, None] & ~torch.eye(B, dtype=torch.bool)
    R = torch.where(ok, torch.sigmoid((s[None, :] - s[:, None]) / tau), torch.zeros((), dtype=torch.float64)).sum(1)
    yt = torch.from_numpy(y)
    G = torch.exp2(yt) - 1.0 if gain == 'exp2' else yt
    rows = torch.arange(B)
    before = (yt[None, :] > yt[:, None]) | ((yt[None, :] == yt[:, None]) & (rows[None, :] < rows[:, None]))
    q = (ok & before).sum(1).to(torch.float64)
    tf = t.to(torch.float64)
    onehot = torch.from_numpy((lid[None, :] == np.arange(lid.max() + 1)[:, None]).astype(np.float64))
    idcg = onehot @ (tf * G / torch.log2(2.0 + q))
    adcg = onehot @ (tf * G / torch.log2(2.0 + R))
    good = idcg > 0
    return -(adcg[good] / idcg[good]).mean()


@pytest.mark.parametrize('tau', [0.1, 1.0])
@pytest.mark.parametrize('gain', ['exp2', 'linear'])
def test_against_torch_autograd_in_fp64(gain, tau):
    rng = np.random.default_rng(5)
    B = 90
    groups = rng.integers(0, 9, B).astype(np.float32)
    g2 = rng.integers(0, 2, B).astype(np.float32)
    s = np.round(rng.normal(size=B) * 16) / 16                      # ties
    y = rng.integers(0, 4, B).astype(np.float64)
    y[groups == 3] = 0.0                                            # a list with IDCG = 0
    mask = rng.random(B) < 0.8
    mask[groups == 5] = False                                       # a list without a taking-part row
    for grp in (groups, [groups, g2]):
        for m in (None, mask):
            res = AO.approx_ndcg(s, y, grp, m, gain, tau)
            assert (~res.valid).any() and res.valid.sum() == res.n_lists
            st = torch.from_numpy(s.copy()).requires_grad_(True)
            take = np.ones(B, dtype=bool) if m is None else m
            loss = _dense(st, y, O.list_ids(grp), take, gain, tau)
            (g,) = torch.autograd.grad(loss, st)
            assert abs(res.loss - loss.item()) <= 1e-12
            assert np.abs(res.grad - g.numpy()).max() <= 1e-12
            assert (res.grad[~take] == 0).all() and (res.grad[np.isin(res.list_id, np.flatnonzero(~res.valid))] == 0).all()


def test_small_temperature_gives_the_hard_ndcg():
    groups, s, y = AO.tie_free_batch([1, 2, 3, 40, 513, 7, 100], 11)
    for rows in O.rows_of_lists(O.list_ids(groups)):
        v = np.sort(s[rows].astype(np.float64))
        assert rows.size < 2 or np.diff(v).min() / 1e-4 >= 39
    mask = np.random.default_rng(3).random(s.size) < 0.8
    for gain in ('exp2', 'linear'):
        for m in (None, mask):
            res = AO.approx_ndcg(s, y, groups, m, gain, 1e-4)
            hard = O.rank_terms(s, y, groups, m, gain)
            assert res.n_lists == hard.n_lists and abs(-res.loss - hard.ndcg_mean) <= 1e-12
            take = np.ones(s.size, dtype=bool) if m is None else m
            assert np.abs(res.approx_rank[take] - hard.rank[take]).max() <= 1e-12


@pytest.mark.parametrize('tau', [0.1, 1.0])
def test_every_list_gradient_sums_to_zero(tau):
    groups, s, y, mask = O.layout('r2049')
    for m in (None, mask):
        res = AO.approx_ndcg(s, y, groups, m, 'exp2', tau)
        for g, rows in enumerate(res.lists):
            top = np.abs(res.grad[rows]).max()
            assert abs(res.grad[rows].sum()) <= 1e-12 * top
            assert res.valid[g] or top == 0


def test_what_the_layouts_hold():
    """From the oracle alone: what the GPU cases have to contain between them."""
    n_valid = {}
    for name in O.LAYOUTS:
        groups, s, y, mask = O.layout(name)
        res = AO.approx_ndcg(s, y, groups, mask, 'exp2', 0.1)
        n_valid[name] = (int(res.valid.sum()), len(res.lists))
        assert any(rows.size == 1 for rows in res.lists)
        assert any(np.unique(s[rows]).size < rows.size for rows in res.lists)          # tied scores
    assert n_valid == {'r2049': (12, 12), 'r2048': (10, 11), 'chain': (8, 8)}


def test_nan_scores_and_rows_that_do_not_take_part():
    groups, s, y, mask = (np.array(a) for a in O.layout('r2049'))
    clean = AO.approx_ndcg(s, y, groups, mask)
    out = np.flatnonzero(~mask)[:7]
    s2, y2 = s.copy(), y.copy()
    s2[out], y2[out[:3]] = np.nan, np.nan
    dirty = AO.approx_ndcg(s2, y2, groups, mask)
    for a, b in zip(clean[:5] + clean[7:], dirty[:5] + dirty[7:]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    row = int(np.flatnonzero(mask & (clean.list_id == clean.list_id[out[0]]))[0])
    s3 = s.copy()
    s3[row] = np.nan
    bad = AO.approx_ndcg(s3, y, groups, mask)
    in_list = clean.list_id == clean.list_id[row]
    assert np.isnan(bad.loss) and np.isnan(bad.grad[in_list & mask]).all() and (bad.grad[in_list & ~mask] == 0).all()
    # the other lists: the same per-list gradient (the division by n_lists is the same)
    assert bad.n_lists == clean.n_lists and bad.grad[~in_list].tobytes() == clean.grad[~in_list].tobytes()
    # a NaN score in a list of one
    one = AO.approx_ndcg(np.array([np.nan, 1.0, 2.0]), np.array([1.0, 1.0, 0.0]), np.array([0, 1, 1]))
    assert np.isnan(one.loss) and np.isnan(one.grad[0]) and np.isfinite(one.grad[1:]).all() and one.n_lists == 2
    # a NaN label makes its list invalid
    lab = AO.approx_ndcg(np.array([0.5, 1.0, 2.0]), np.array([np.nan, 1.0, 0.0]), np.array([0, 1, 1]))
    assert lab.n_lists == 1 and not lab.valid[0] and lab.grad[0] == 0 and np.isfinite(lab.loss)


def test_argument_errors_need_no_device():
    from rec_now_amd.rec_block import approx_ndcg as M
    s, y, g = torch.zeros(6), torch.zeros(6), torch.zeros(6)
    with pytest.raises(ValueError, match='gain'):
        M.approx_ndcg_loss(s, y, g, gain='exp')
    with pytest.raises(ValueError, match='gain'):
        M.approx_ndcg_terms(s, y, g, gain=0)
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), True, None, '0.1'):
        with pytest.raises(ValueError, match='temperature'):
            M.approx_ndcg_loss(s, y, g, temperature=bad)
        with pytest.raises(ValueError, match='temperature'):
            M.approx_ndcg_terms(s, y, g, temperature=bad)
    with pytest.raises(ValueError, match='same number of elements'):
        M.approx_ndcg_loss(torch.zeros(5), y, g)
    with pytest.raises(ValueError, match='same number of elements'):
        M.approx_ndcg_loss(s, torch.zeros(7), g)
    with pytest.raises(ValueError, match='same number of elements'):
        M.approx_ndcg_terms(s, y, g, mask=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match='same number of elements'):
        M.approx_ndcg_loss(s, y, [g, torch.zeros(4)])
    assert M.ApproxNDCGTerms._fields == ('approx_rank', 'list_adcg', 'list_idcg', 'loss_sum', 'n_lists')

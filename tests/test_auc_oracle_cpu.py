"""CPU: the numpy oracle of the in-batch GAUC (tests/_auc_oracle.py) pinned three ways -- to a batch worked by hand, to a dense brute force over
all pairs, and, for 0/1 labels, to the midrank Mann-Whitney statistic -- with exact counts and the AUC within 1e-12; the argument checks of
rec_block/auc.py; dp.global_gauc without a process group."""
import numpy as np
import pytest
import torch

import _auc_oracle as A

NAN = float('nan')


# ---- a batch worked by hand ---------------------------------------------------------------------------------------------------------------
# list 0 (rows 0..7): tied scores (rows 0 and 1 at 0.9, rows 3 and 7 at 0.7, rows 2 and 6 at 0.5), row 5 masked out, row 4 has a NaN score.
# list 1 (rows 8, 9): equal labels, no pair.   list 2 (rows 10..12): one positive between two negatives.
#          row:   0    1    2    3    4    5    6    7    8    9    10   11   12
H_GROUPS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2]
H_LABELS = [1, 0, 1, 0, 1, 0, 0, 2, 1, 1, 1, 0, 0]
H_SCORES = [.9, .9, .5, .7, NAN, .1, .5, .7, .3, .6, .3, .2, .4]
H_MASK = [1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1]


def _hand(th):
    return A.counts(np.array(H_SCORES, dtype=np.float32), np.array(H_LABELS, dtype=np.float32), np.array(H_GROUPS, dtype=np.float32),
                    np.array(H_MASK, dtype=bool), th)


def test_hand_worked_graded():
    c = _hand(None)
    # row 0 (label 1, 0.9) over the label-0 rows 1 (0.9: tie), 3 (0.7) and 6 (0.5); row 2 (0.5) over 1, 3 (both higher) and 6 (tie); row 4 (NaN):
    # three pairs, none concordant, none tied; row 7 (label 2, 0.7) over rows 0, 1 (higher), 2, 6 (lower), 3 (tie) and 4 (NaN: discordant);
    # row 5 is masked out and is nobody's partner
    assert c.row_n.tolist() == [3, 0, 3, 0, 3, 0, 0, 6, 0, 0, 2, 0, 0]
    assert c.row_c.tolist() == [2, 0, 0, 0, 0, 0, 0, 2, 0, 0, 1, 0, 0]
    assert c.row_t.tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert c.N.tolist() == [15, 0, 2] and c.C.tolist() == [4, 0, 1] and c.T.tolist() == [3, 0, 0] and c.R.tolist() == [7, 2, 3]
    assert abs(c.auc[0] - 11.0 / 30.0) <= 1e-12 and np.isnan(c.auc[1]) and c.auc[2] == 0.5
    rows, pairs, uni = (A.metric(c, w) for w in A.WEIGHTS)
    assert rows.n_lists == pairs.n_lists == uni.n_lists == 2
    assert abs(rows.weighted_sum - (7 * 11.0 / 30.0 + 1.5)) <= 1e-12 and rows.weight_sum == 10.0
    assert abs(rows.auc - (7 * 11.0 / 30.0 + 1.5) / 10.0) <= 1e-12
    assert abs(pairs.auc - 6.5 / 17.0) <= 1e-12 and pairs.weight_sum == 17.0       # (2 * 5 + 3) / (2 * 17): the pooled share
    assert abs(uni.auc - (11.0 / 30.0 + 0.5) / 2.0) <= 1e-12 and uni.weight_sum == 2.0


def test_hand_worked_binary():
    c = _hand(0.5)                                   # positives: labels 1 and 2; row 7 now stands over the label-0 rows 1, 3, 6 only
    assert c.row_n.tolist() == [3, 0, 3, 0, 3, 0, 0, 3, 0, 0, 2, 0, 0]
    assert c.row_c.tolist() == [2, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    assert c.row_t.tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert c.N.tolist() == [12, 0, 2] and c.C.tolist() == [3, 0, 1] and c.T.tolist() == [3, 0, 0]
    assert c.auc[0] == 0.375 and c.auc[2] == 0.5
    c = _hand(1.5)                                   # the only positive is row 7; lists 1 and 2 have none
    assert c.row_n.tolist() == [0, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0]
    assert c.N.tolist() == [6, 0, 0] and c.C.tolist() == [2, 0, 0] and c.T.tolist() == [1, 0, 0] and c.R.tolist() == [7, 2, 3]
    assert abs(c.auc[0] - 5.0 / 12.0) <= 1e-12
    m = A.metric(c, 'rows')
    assert m.n_lists == 1 and m.weight_sum == 7.0 and abs(m.auc - 5.0 / 12.0) <= 1e-12


def test_nan_label_and_empty_metric():
    s = np.array([3, 2, 1, 0], dtype=np.float32)
    y = np.array([NAN, 1, 0, 0], dtype=np.float32)
    g = np.zeros(4, dtype=np.float32)
    assert A.counts(s, y, g).row_n.tolist() == [0, 2, 0, 0]                        # graded: a NaN label is in no pair
    assert A.counts(s, y, g, pos_neg_th=0.5).row_n.tolist() == [0, 3, 0, 0]        # binary: it is a negative
    none = A.metric(A.counts(s, np.ones(4, dtype=np.float32), g))
    assert none == A.Metric(0.0, 0, 0.0, 0.0)
    empty = A.counts(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32))
    assert empty.row_n.size == 0 and A.metric(empty).n_lists == 0


# ---- dense brute force ----------------------------------------------------------------------------------------------------------------------
def _batch(seed, B=203, n_groups=9, levels=4):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, n_groups, B).astype(np.float32)
    g2 = rng.integers(0, 2, B).astype(np.float32)
    s = (np.round(rng.normal(size=B) * 8) / 8).astype(np.float32)                  # many ties
    s[rng.integers(0, B, 3)] = np.nan
    y = rng.integers(0, levels, B).astype(np.float32)
    mask = rng.random(B) < 0.8
    return g, g2, s, y, mask


@pytest.mark.parametrize('th', [None, 0.5, 1.5])
@pytest.mark.parametrize('two', [False, True])
def test_dense_brute_force(th, two):
    g, g2, s, y, mask = _batch(11)
    groups = [g, g2] if two else g
    c = A.counts(s, y, groups, mask, th)
    B = s.size
    same = g[:, None] == g[None, :]
    if two:
        same &= g2[:, None] == g2[None, :]
    with np.errstate(invalid='ignore'):
        rule = (y[:, None] > y[None, :]) if th is None else ((y[:, None] > np.float32(th)) & ~(y[None, :] > np.float32(th)))
        pair = same & rule & mask[:, None] & mask[None, :] & ~np.eye(B, dtype=bool)
        conc, tied = pair & (s[:, None] > s[None, :]), pair & (s[:, None] == s[None, :])
    assert np.array_equal(c.row_n, pair.sum(1)) and np.array_equal(c.row_c, conc.sum(1)) and np.array_equal(c.row_t, tied.sum(1))
    assert c.row_n.sum() > 0 and c.row_t.sum() > 0 and (c.row_n - c.row_c - c.row_t).sum() > 0
    assert len(c.lists) == (18 if two else 9)
    for k, rows in enumerate(c.lists):
        assert (c.list_id[rows] == k).all()
        N, C, T = int(pair[rows].sum()), int(conc[rows].sum()), int(tied[rows].sum())
        assert (c.N[k], c.C[k], c.T[k], c.R[k]) == (N, C, T, int(mask[rows].sum()))
        if N:
            assert abs(c.auc[k] - (C + 0.5 * T) / N) <= 1e-12
        else:
            assert np.isnan(c.auc[k])
    for w in A.WEIGHTS:
        ok = c.N > 0
        wl = {'rows': c.R, 'pairs': c.N, 'uniform': np.ones_like(c.N)}[w][ok].astype(np.float64)
        m = A.metric(c, w)
        assert m.n_lists == int(ok.sum())
        assert abs(m.auc - float((wl * c.auc[ok]).sum() / wl.sum())) <= 1e-12
    pooled = A.metric(c, 'pairs')
    assert abs(pooled.auc - (2 * int(c.C.sum()) + int(c.T.sum())) / (2.0 * int(c.N.sum()))) <= 1e-12


# ---- Mann-Whitney ---------------------------------------------------------------------------------------------------------------------------
def _midranks(v):
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    hi = np.cumsum(cnt).astype(np.float64)
    return (hi - (cnt - 1) / 2.0)[inv.reshape(-1)]


@pytest.mark.parametrize('th', [None, 0.5])
def test_midrank_mann_whitney(th):
    rng = np.random.default_rng(5)
    B = 400
    g = rng.integers(0, 7, B).astype(np.float32)
    s = (np.round(rng.normal(size=B) * 4) / 4).astype(np.float32)
    y = (rng.random(B) < 0.3).astype(np.float32)
    y[g == 6] = 0.0                                               # a list without a positive
    c = A.counts(s, y, g, None, th)
    seen = 0
    for k, rows in enumerate(c.lists):
        pos = y[rows] > 0
        P, Q = int(pos.sum()), int((~pos).sum())
        assert c.N[k] == P * Q
        if P * Q == 0:
            assert np.isnan(c.auc[k])
            continue
        u = _midranks(s[rows])[pos].sum() - P * (P + 1) / 2.0
        assert abs(c.auc[k] - u / (P * Q)) <= 1e-12
        seen += 1
    assert seen == 6 and c.T.sum() > 0


# ---- argument checks and the data-parallel combination ------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [{'weight': 'mean'}, {'weight': None}, {'weight': 0}, {'pos_neg_th': True}, {'pos_neg_th': '0.5'},
                                {'pos_neg_th': NAN}, {'pos_neg_th': float('inf')}, {'pos_neg_th': torch.tensor(0.5)}])
def test_argument_checks(kw):
    from rec_now_amd.rec_block import auc
    z = torch.zeros(4)
    with pytest.raises(ValueError):
        auc.in_batch_gauc(z, z, z, **kw)
    if 'weight' not in kw:
        with pytest.raises(ValueError):
            auc.auc_terms(z, z, z, **kw)


def test_accepted_options_reach_the_gpu_check():
    """valid options pass the argument checks: the call then stops at the CPU tensor, loudly"""
    from rec_now_amd.rec_block import auc
    z = torch.zeros(4)
    for kw in ({}, {'weight': 'pairs', 'pos_neg_th': 0.5}, {'weight': 'uniform', 'pos_neg_th': 1}, {'pos_neg_th': np.float32(1.5)}):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            auc.in_batch_gauc(z, z, z, **kw)


def test_global_gauc_without_a_process_group():
    from rec_now_amd import dp
    gauc, n = dp.global_gauc(torch.tensor(5.2, dtype=torch.float64), torch.tensor(10.0, dtype=torch.float64), torch.tensor(2))
    assert gauc.dtype == torch.float64 and n.dtype == torch.int64
    assert gauc.item() == 5.2 / 10.0 and n.item() == 2
    gauc, n = dp.global_gauc(torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64), torch.tensor(0))
    assert gauc.item() == 0.0 and n.item() == 0

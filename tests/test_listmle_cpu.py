"""CPU: the fp64 oracle of the in-batch ListMLE loss (tests/_listmle_oracle.py) pinned three ways, and the argument errors of
rec_now_amd.rec_block.listmle that need no device.

The list worked by hand.  Three rows of one list, labels (1, 3, 2), logits (ln 1, ln 2, ln 3).  The permutation is row 1, row 2, row 0 with
exp(s) = 2, 3, 1, so
  lse_1 = ln 6, lse_2 = ln 4, lse_3 = ln 1          P(permutation) = 2/6 * 3/4 * 1/1 = 1/4
  loss  = (ln 6 - ln 2) + (ln 4 - ln 3) + 0 = ln 4
  A_1 = 1/6, A_2 = 1/6 + 1/4 = 5/12, A_3 = 5/12 + 1 = 17/12
  gradient by place: 2 * 1/6 - 1 = -2/3,  3 * 5/12 - 1 = 1/4,  1 * 17/12 - 1 = 5/12     (sum 0);  by row: (5/12, -2/3, 1/4)
  topn = 1:  loss = ln 6 - ln 2 = ln 3,  gradient by place 2/6 - 1, 3/6, 1/6;  by row: (1/6, -2/3, 1/2).

Large logits are logits around +120 or -120, list by list, with a spread of 1 inside a list.  With a spread of tens of units at that magnitude
a list that already stands in label order has gradients near exp(-gap), while fp64 rounds s - lse at ulp(120) = 1.4e-14: the oracle and
torch.logcumsumexp autograd then differ by more than 1e-12 of the list's largest entry."""
import numpy as np
import pytest
import torch

import _listmle_oracle as MO
from _listwise_oracle import list_index


def test_oracle_on_the_list_worked_by_hand():
    ids, y, s = np.zeros(3, np.int64), np.array([1, 3, 2], np.float32), np.log(np.array([1.0, 2.0, 3.0])).astype(np.float32)
    r = MO.listmle_ref(ids, y, s)
    assert r.n_valid == 1 and r.valid.tolist() == [True] and r.position.tolist() == [2, 0, 1]
    np.testing.assert_allclose(r.loss, np.log(4.0), rtol=1e-7)                    # (the logits are float32 roundings of ln 2, ln 3)
    np.testing.assert_allclose(r.lse, [0.0, np.log(6.0), np.log(4.0)], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(r.grad, [5 / 12, -2 / 3, 1 / 4], rtol=1e-6)
    r1 = MO.listmle_ref(ids, y, s, topn=1)
    np.testing.assert_allclose(r1.loss, np.log(3.0), rtol=1e-7)
    np.testing.assert_allclose(r1.grad, [1 / 6, -2 / 3, 1 / 2], rtol=1e-6)
    rm = MO.listmle_ref(ids, y, s, topn=2, list_mean=True, weights=np.array([3.0]))
    np.testing.assert_allclose(rm.loss, 3.0 * np.log(4.0) / 2, rtol=1e-7)         # (place 3 adds 0: the top-2 loss is ln 4 as well)


def _case(seed, B=200, G=23, offset=0.0, distinct=False):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, G, B).astype(np.int64)
    ids[:3] = G + np.arange(3)                                                    # single-row lists
    y = (rng.normal(size=B) if distinct else rng.integers(0, 4, B)).astype(np.float32)
    y[ids == 5] = 2.0                                                             # a list with all labels equal
    y[rng.random(B) < 0.05] = np.nan
    y[np.nonzero(y == 0)[0][::2]] = -0.0
    s = (rng.normal(size=B) + offset * np.where(ids % 2 == 0, 1.0, -1.0)).astype(np.float32)      # logits around +offset or -offset, list by list
    mask = (rng.random(B) < 0.85).astype(np.uint8)
    mask[ids == 7] = 0                                                            # a list with every row masked
    return ids, y, s, mask


def _permutations(ids, y, mask):
    """[(list index, rows in permutation order)] through one lexsort: another route to the order than the oracle's per-list argsort."""
    row_list, G = list_index(ids)
    part = ~np.isnan(y) & (mask != 0 if mask is not None else True)
    rows = np.nonzero(part)[0]
    key = -(y[rows].astype(np.float64) + 0.0)
    o = rows[np.lexsort((rows, key, row_list[rows]))]
    return [(g, o[row_list[o] == g]) for g in range(G)], row_list


@pytest.mark.parametrize('topn', [None, 1, 3])
def test_oracle_against_the_product_of_softmax_choices(topn):
    ids, y, s, mask = _case(1)
    r = MO.listmle_ref(ids, y, s, mask=mask, topn=topn)
    perms, _ = _permutations(ids, y, mask)
    assert r.n_valid >= 8 and (~r.valid).sum() >= 5
    for g, perm in perms:
        sp = s[perm].astype(np.float64)
        K = perm.size if topn is None else min(topn, perm.size)
        prob = 1.0
        for p in range(K):
            prob *= np.exp(sp[p]) / np.exp(sp[p:]).sum()
        assert abs(r.list_loss[g] - (-np.log(prob))) <= 1e-12 * max(1.0, abs(np.log(prob))), (g, perm.size)
        assert np.array_equal(r.position[perm], np.arange(perm.size))


@pytest.mark.parametrize('topn', [None, 1, 3])
@pytest.mark.parametrize('offset,distinct,list_mean,weighted,masked', [(1.0, False, False, False, True), (120.0, False, True, True, True),
                                                                      (1.0, True, True, False, False), (120.0, True, False, True, False)])
def test_oracle_against_logcumsumexp_autograd(topn, offset, distinct, list_mean, weighted, masked):
    ids, y, s, mask = _case(2 if distinct else 3, offset=offset, distinct=distinct)
    mask = mask if masked else None
    perms, row_list = _permutations(ids, y, mask)
    valid = [perm.size >= 2 and np.unique(y[perm].astype(np.float64) + 0.0).size >= 2 for _, perm in perms]
    nv = int(np.sum(valid))
    w = np.random.default_rng(9).uniform(0.5, 2.0, nv) if weighted else None
    r = MO.listmle_ref(ids, y, s, weights=w, mask=mask, topn=topn, list_mean=list_mean)
    assert r.n_valid == nv and r.valid.tolist() == valid and nv >= 8
    st = torch.tensor(s.astype(np.float64), requires_grad=True)
    losses = []
    for (g, perm), v in zip(perms, valid):
        if not v:
            continue
        sp = st[torch.from_numpy(perm)]
        K = perm.size if topn is None else min(topn, perm.size)
        lse = torch.logcumsumexp(sp.flip(0), 0).flip(0)
        np.testing.assert_allclose(r.lse[perm], lse.detach().numpy(), rtol=1e-12, atol=1e-12)
        l = (lse[:K] - sp[:K]).sum()
        assert abs(r.list_loss[g] - float(l.detach())) <= 1e-12 * max(1.0, abs(float(l.detach())))
        losses.append(l * (1.0 / K if list_mean else 1.0) * (w[len(losses)] if weighted else 1.0))
    per_list = torch.stack(losses)
    per_list.mean().backward()
    np.testing.assert_allclose(r.per_list, per_list.detach().numpy(), rtol=1e-12)
    assert abs(r.loss - float(per_list.detach().mean())) <= 1e-12 * abs(float(per_list.detach().mean()))
    g = st.grad.numpy()
    big = np.zeros(r.valid.size)
    np.maximum.at(big, row_list, np.abs(g))
    assert (np.abs(r.grad - g) <= 1e-12 * np.maximum(big[row_list], 1e-300)).all()
    sums = np.bincount(row_list, weights=r.grad, minlength=r.valid.size)
    assert (np.abs(sums) <= 1e-12 * big).all()                                    # the gradient of every list sums to zero
    assert not r.grad[~r.valid[row_list]].any()


def test_oracle_ties_and_non_finite_logits():
    ids = np.array([4, 4, 9, 4, 9, 4, 9], np.int64)
    y = np.array([1, 2, 0, 1, 1, 2, 0], np.float32)
    s = np.array([0.5, -1.0, 0.25, 2.0, np.inf, 0.0, 1.0], np.float32)
    r = MO.listmle_ref(ids, y, s)
    assert r.position.tolist() == [2, 0, 1, 3, 0, 1, 2]                            # ties by ascending row index
    assert r.valid.tolist() == [True, True] and np.isnan(r.list_loss[1]) and np.isfinite(r.list_loss[0])
    assert np.isnan(r.grad[[2, 4, 6]]).all() and np.isfinite(r.grad[[0, 1, 3, 5]]).all()


# ---- the public function: what it refuses without a device ---------------------------------------------------------------------------------------
def _fn():
    from rec_now_amd.rec_block.listmle import listmle_loss_from_batch, listmle_terms
    return listmle_loss_from_batch, listmle_terms


def test_argument_errors_need_no_device():
    loss, terms = _fn()
    g, y, s = torch.zeros(6, dtype=torch.int64), torch.zeros(6), torch.zeros(6)
    with pytest.raises(ValueError, match='same number of elements'):
        loss(g, y[:5], s)
    with pytest.raises(ValueError, match='same number of elements'):
        loss(g, y, torch.zeros(7))
    with pytest.raises(ValueError, match='same number of elements'):
        loss(g, y, s, mask=torch.ones(4))
    with pytest.raises(ValueError, match='same number of elements'):
        loss([g, g[:5]], y, s)
    with pytest.raises(ValueError, match='same number of elements'):
        terms(g, y[:5], s)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match='topn'):
            loss(g, y, s, topn=bad)
        with pytest.raises(ValueError, match='topn'):
            terms(g, y, s, topn=bad)
    with pytest.raises(ValueError, match='one entry per valid list'):
        loss(g, y, s, weights=torch.ones(7), do_reduce=False)                     # more weights than rows: wrong whatever the lists are


def test_cpu_tensors_are_refused_loudly():
    loss, terms = _fn()
    g, y, s = torch.zeros(6, dtype=torch.int64), torch.zeros(6), torch.zeros(6, requires_grad=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        loss(g, y, s)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        terms(g, y, s)


def test_abi_23_binds_the_listmle_entries():
    from rec_now_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 23 and lib.recnow_abi_version() == _lib.ABI_VERSION
    assert lib.recnow_listmle_workspace_bytes(-1) == 0
    small, big = lib.recnow_listmle_workspace_bytes(0), lib.recnow_listmle_workspace_bytes(65536)
    assert 0 < small < big < 65536 * 256                                          # sized by B alone, well under 256 bytes a row
    # B < 0 and topn < 0 are refused before any pointer is looked at; B == 0 with no output asked for touches no device
    assert lib.recnow_listmle_fwdbwd(*([None] * 8), -1, 0, 0, 0, *([None] * 10), 0, None) == -1
    assert lib.recnow_listmle_fwdbwd(*([None] * 8), 4, -1, 0, 0, *([None] * 10), 0, None) == -1
    assert lib.recnow_listmle_fwdbwd(*([None] * 8), 0, 0, 0, 0, *([None] * 10), 0, None) == 0

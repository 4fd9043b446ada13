"""Dense fp64 oracle of the NDCG (LambdaRank) pair weight, the in-batch NDCG and the pairwise loss that carries the weight, written from the
definitions alone (numpy for the ranks and list sums, torch fp64 for the loss so that autograd gives the gradient).  It is never the code
under test and calls nothing of rec_now_amd.  Also the batches the CPU and GPU tests share.

  list      the rows that agree in every group tensor; only rows that take part (mask true, or no mask) are ranked
  position  r_i = #{ j in the list, taking part, j != i : s_j > s_i or (s_j == s_i and j < i) }   (q_i: the same on the labels)
  D(r) = 1 / log2(2 + r), 0 for r >= topn;   G(y) = 2**y - 1 ('exp2') or y ('linear')
  DCG = sum G(y_i) D(r_i), IDCG = sum G(y_i) D(q_i), inv = 1 / IDCG where IDCG > 0 else 0
  lambda_ij = |G(y_i) - G(y_j)| |D(r_i) - D(r_j)| inv(list);   metric: mean of DCG / IDCG over the lists with IDCG > 0, and their number
The weight multiplies a pair's term beside the rule weight and the occurrence weight; it never changes which pairs exist."""
import collections

import numpy as np
import torch

LEVELS = [0.0, 1.0, 2.0, 3.0]
KINK = 2.0 ** -10


def _as_list(g):
    return list(g) if isinstance(g, (list, tuple)) else [g]


def list_ids(groups):
    """(B,) int64: rows with the same value agree in every group tensor (exact for any id dtype: each tensor is ranked on its own)."""
    lid = None
    for t in _as_list(groups):
        _, inv = np.unique(np.asarray(t).reshape(-1), return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        lid = inv if lid is None else lid * (int(inv.max()) + 1 if inv.size else 1) + inv
    return lid


def _positions(v, rows, take):
    """positions of the taking-part rows by value v (descending, ties to the smaller original row index); -1 elsewhere"""
    before = (v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (rows[None, :] < rows[:, None]))      # [i, j]: j stands before i
    before &= take[None, :]
    np.fill_diagonal(before, False)
    return np.where(take, before.sum(1), -1)


def discount(r, topn=None):
    r = np.asarray(r, dtype=np.float64)
    d = 1.0 / np.log2(2.0 + np.maximum(r, 0.0))
    if topn is not None:
        d = np.where(r >= topn, 0.0, d)
    return d


def gain_of(y, gain='exp2'):
    y = np.asarray(y, dtype=np.float64)
    return np.exp2(y) - 1.0 if gain == 'exp2' else y


Terms = collections.namedtuple('Terms', ['rank', 'qrank', 'discount', 'gain', 'inv_idcg', 'list_id', 'dcg', 'idcg', 'ndcg_mean', 'n_lists'])


def rank_terms(scores, labels, groups, mask=None, gain='exp2', topn=None):
    """Per original row: rank (-1 for a row that does not take part), qrank, D(rank), G(label) (both 0 for such a row), inv of the row's list;
    per list (in the order of list_id): DCG, IDCG; the batch metric and the number of lists with IDCG > 0."""
    s = np.asarray(scores).reshape(-1).astype(np.float64)           # float32 values, compared exactly
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    B = s.size
    take_all = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    lid = list_ids(groups) if B else np.zeros(0, dtype=np.int64)
    _, lid = np.unique(lid, return_inverse=True)
    lid = lid.reshape(-1)
    n_list = int(lid.max()) + 1 if B else 0
    rank, qrank = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    disc, gn, inv = np.zeros(B), np.zeros(B), np.zeros(B)
    dcg, idcg = np.zeros(n_list), np.zeros(n_list)
    for g in range(n_list):
        rows = np.flatnonzero(lid == g)
        take = take_all[rows]
        r = _positions(s[rows], rows, take)
        q = _positions(y[rows], rows, take)
        G = np.where(take, gain_of(y[rows], gain), 0.0)
        D = np.where(take, discount(r, topn), 0.0)
        Dq = np.where(take, discount(q, topn), 0.0)
        rank[rows], qrank[rows], disc[rows], gn[rows] = r, q, D, G
        dcg[g], idcg[g] = (G * D).sum(), (G * Dq).sum()
        inv[rows] = 1.0 / idcg[g] if idcg[g] > 0 else 0.0
    good = idcg > 0
    mean = float((dcg[good] / idcg[good]).mean()) if good.any() else 0.0
    return Terms(rank, qrank, disc, gn, inv, lid, dcg, idcg, mean, int(good.sum()))


def pairwise_loss(outputs, labels, groups, pairloss_func, only_use_wrong_order_pair=False, click_occurance_power=0.0, mask=None,
                  label_pair_to_weight_func=None, lam=None):
    """(loss, number of pairs).  outputs: fp64 torch tensor (requires_grad for the gradient); labels, groups, mask: numpy.
    Pairs (i, j): same list, i != j, both take part, rule weight > 0 (label_i > label_j with weight 1 when no function is given), and
    s_i < s_j under only_use_wrong_order_pair; in row-major order.  weight = rule weight * (pairs whose positive row shares i's main group)
    ** power * lambda_ij, each factor only where it applies, all constants.  lam: None or (gain, topn)."""
    s = outputs.reshape(-1)
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    B = y.size
    lid = list_ids(groups)
    pm = lid[:, None] == lid[None, :]
    np.fill_diagonal(pm, False)
    if mask is not None:
        m = np.asarray(mask).reshape(-1).astype(bool)
        pm &= m[:, None] & m[None, :]
    W = None
    if label_pair_to_weight_func is None:
        pm &= y[:, None] > y[None, :]
    else:
        yt = torch.from_numpy(y)
        W = label_pair_to_weight_func(yt.reshape(-1, 1).expand(B, B), yt.reshape(1, -1).expand(B, B)).numpy()
        pm &= W > 0
    if only_use_wrong_order_pair:
        sv = s.detach().numpy()
        pm &= sv[:, None] < sv[None, :]
    i, j = np.nonzero(pm)
    weights = None
    if W is not None:
        weights = W[i, j].astype(np.float64)
    if click_occurance_power != 0.0:
        main = list_ids(_as_list(groups)[0])[i]
        # the reference forms count ** power in float32 (rec_now/rec_block/pairwise_loss_from_batch.py:130-151); that rounding is part of the contract
        cnt = torch.from_numpy(np.bincount(main, minlength=1)[main]).to(torch.float32)
        occ = (cnt if click_occurance_power == 1.0 else torch.pow(cnt, click_occurance_power)).numpy().astype(np.float64)
        weights = occ if weights is None else weights * occ
    if lam is not None:
        t = rank_terms(s.detach().numpy(), y, groups, mask, lam[0], lam[1])
        lw = np.abs(t.gain[i] - t.gain[j]) * np.abs(t.discount[i] - t.discount[j]) * t.inv_idcg[i]
        weights = lw if weights is None else weights * lw
    wt = None if weights is None else torch.from_numpy(weights)
    it, jt = torch.from_numpy(i), torch.from_numpy(j)
    return pairloss_func(s[it], s[jt], wt), float(i.size)


# ---- the pair losses, restated in fp64 torch ---------------------------------------------------------------------------------------------
def ref_loss(kind, margin=0.0, factor=1.0, reduce_mean=True):
    """kind 'bpr': softplus(-factor (pos - neg)); 'hinge' / 'squared_hinge' / 'margin_bpr': f(margin - factor (pos - neg))."""
    def loss(pos, neg, weights=None):
        u = (margin if kind != 'bpr' else 0.0) - factor * (pos - neg)
        if kind == 'hinge':
            t = torch.relu(u)
        elif kind == 'squared_hinge':
            t = torch.relu(u) * torch.relu(u)
        else:
            t = torch.logaddexp(u, torch.zeros_like(u))           # softplus, smooth at u == 0
        n = t.numel()
        if weights is not None:
            t = t * weights
        return t.sum() / (n + 1e-10) if reduce_mean else t.sum()
    return loss


def w_sym(a, b, **k):                            # both directions, tied labels are pairs
    return (a - b).abs() + 0.5


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def batch(name):
    """(groups, scores, labels, mask) as read-only numpy; scores = round(N(0, 1) * 256) / 256 (the large groups are full of ties), labels in
    {0, 1, 2, 3}, the mask keeps ~80 % of the rows.  b2900: one group of 2100 rows (beyond PW_STAGE = 2048: global-memory walk), one of 600
    (beyond PW_LONG = 512: a wave per row inside LDS) and 200 rows in small groups."""
    if name in _BATCHES:
        return _BATCHES[name]
    seed = {'b1': 11, 'b2': 12, 'b64': 13, 'b1000': 14, 'b2900': 15}[name]
    rng = np.random.default_rng(seed)
    if name == 'b2900':
        groups = np.concatenate([np.zeros(2100), np.ones(600), rng.integers(2, 22, 200)]).astype(np.float32)
        rng.shuffle(groups)
    else:
        B, G = {'b1': (1, 1), 'b2': (2, 1), 'b64': (64, 4), 'b1000': (1000, 17)}[name]
        groups = rng.integers(0, G, B).astype(np.float32)
    B = groups.size
    scores = (np.round(rng.normal(size=B) * 256) / 256).astype(np.float32)
    labels = rng.integers(0, 4, B).astype(np.float32)
    mask = rng.random(B) < 0.8
    if name in ('b1', 'b2'):
        mask = np.ones(B, dtype=bool)
    if name == 'b2':
        labels = np.array([1.0, 3.0], dtype=np.float32)
    for a in (groups, scores, labels, mask):
        a.setflags(write=False)
    _BATCHES[name] = (groups, scores, labels, mask)
    return _BATCHES[name]


def hand_made(name):
    """Four hand-made batches of three lists each: the named list (group 0, 40 rows) beside two ordinary ones (groups 1 and 2, 30 rows each).
      'equal'    every score of list 0 is the same: positions follow the row index alone
      'masked'   every row of list 0 is masked out: no positions, DCG = IDCG = 0
      'single'   exactly one row of list 0 takes part
      'zeros'    every label of list 0 is 0: IDCG = 0, every lambda is 0, the list is left out of the metric"""
    key = 'hand_' + name
    if key in _BATCHES:
        return _BATCHES[key]
    rng = np.random.default_rng({'equal': 21, 'masked': 22, 'single': 23, 'zeros': 24}[name])
    groups = np.concatenate([np.zeros(40), np.ones(30), np.full(30, 2.0)]).astype(np.float32)
    rng.shuffle(groups)
    B = groups.size
    scores = (np.round(rng.normal(size=B) * 256) / 256).astype(np.float32)
    labels = rng.integers(0, 4, B).astype(np.float32)
    mask = rng.random(B) < 0.8
    first = groups == 0
    if name == 'equal':
        scores[first] = 0.25
    elif name == 'masked':
        mask[first] = False
    elif name == 'single':
        mask[first] = False
        mask[np.flatnonzero(first)[7]] = True
    else:
        labels[first] = 0.0
    for a in (groups, scores, labels, mask):
        a.setflags(write=False)
    _BATCHES[key] = (groups, scores, labels, mask)
    return _BATCHES[key]


def second_groups(B):
    g2 = np.random.default_rng(77).integers(0, 3, B).astype(np.float32)
    g2.setflags(write=False)
    return g2


def assert_off_the_kink(groups, scores, margin, factor):
    """From the fp64 values alone: no same-list candidate (i, j), i != j, has |margin - factor (s_i - s_j)| below 2**-10."""
    lid = list_ids(groups)
    if lid.size < 2:
        return
    same = lid[:, None] == lid[None, :]
    np.fill_diagonal(same, False)
    if not same.any():
        return
    s64 = np.asarray(scores).astype(np.float64)
    u = margin - factor * (s64.reshape(-1, 1) - s64.reshape(1, -1))
    assert np.abs(u[same]).min() >= KINK

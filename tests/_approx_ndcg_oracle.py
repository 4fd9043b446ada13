"""Per-list fp64 oracle of the in-batch ApproxNDCG loss (rec_block/approx_ndcg.py), written from the definitions, list by list.  It never forms
more than a 512 x n block of one list and calls nothing of rec_now_amd.  From _pair_lists_oracle it takes the lists, the label positions, the
discount, the gain, the layouts and the census.  tests/test_approx_ndcg_cpu.py pins it.

  lists and rows   a list is the rows that agree in every group tensor; a row takes part when mask is true there, or when there is no mask.
                   Rows that do not take part influence nothing and get gradient exactly 0.
  temperature      tau, a finite float greater than 0
  soft position    R_i = sum_{j in the list, taking part, j != i} sigma((s_j - s_i) / tau); 0-based, so it matches D(r) = 1 / log2(2 + r)
  gain             G(y) = 2**y - 1 ('exp2') or y ('linear')
  ideal DCG        IDCG = sum G(y_i) D(q_i), q_i the label position (ties go to the smaller original row index); no topn
  valid list       IDCG > 0; a NaN label of a taking-part row makes that comparison false, so the list is invalid
  list loss        l = -ADCG / IDCG, ADCG = sum_i G(y_i) / log2(2 + R_i); the batch loss is the mean of l over the valid lists, 0 when none
  gradient         c_i = G(y_i) ln 2 / ((2 + R_i) ln^2(2 + R_i));  sigma'_kj = sigma(x)(1 - sigma(x)), x = (s_j - s_k) / tau;
                   dl/ds_k = (1 / (tau IDCG)) sum_{j != k, taking part} sigma'_kj (c_j - c_k); rows of an invalid list get exactly 0
  NaN scores       a NaN score of a taking-part row makes its own list's loss NaN (its R is NaN, also in a list of one) and the batch mean with
                   it; that list's taking-part rows get NaN gradients; nothing else changes.  A row that does not take part may hold anything.
The gradient returned is that of the batch loss: dl/ds_k divided by the number of valid lists."""
import collections

import numpy as np

import _pair_lists_oracle as O

CHUNK = O.CHUNK
LN2 = float(np.log(2.0))

Result = collections.namedtuple('Result', ['loss', 'loss_sum', 'n_lists', 'grad', 'approx_rank', 'list_id', 'lists', 'adcg', 'idcg', 'valid',
                                           'list_loss'])


def _sigmoid_block(s, a, b, tau):
    """sigma(x) and sigma'(x) for x = (s_j - s_i) / tau, i in [a, b), all j of the list: two (b - a, n) blocks"""
    x = (s[None, :] - s[a:b, None]) / tau
    lp, lm = np.logaddexp(0.0, -x), np.logaddexp(0.0, x)          # -log sigma(x), -log sigma(-x)
    return np.exp(-lp), np.exp(-lp - lm)


def list_terms(s, y, rows, take, gain, tau):
    """One list.  (R, G, q, c, IDCG, ADCG) with R NaN and G, c 0 for the rows that do not take part."""
    n = s.size
    R = np.zeros(n)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, n, CHUNK):
            b = min(n, a + CHUNK)
            sg, _ = _sigmoid_block(s, a, b, tau)
            ok = np.broadcast_to(take[None, :], sg.shape).copy()
            ok[np.arange(b - a), np.arange(a, b)] = False
            R[a:b] = np.where(ok, sg, 0.0).sum(1)
        R = np.where(np.isnan(s), np.nan, R)
        G = np.where(take, O.gain_of(y, gain), 0.0)
        q = O._positions(y, rows, take)
        idcg = float(np.where(take, G * O.discount(q), 0.0).sum())
        L = np.log(2.0 + R)
        adcg = float(np.where(take, G * LN2 / L, 0.0).sum())
        c = np.where(take, G * LN2 / ((2.0 + R) * L * L), 0.0)
    return np.where(take, R, np.nan), G, q, c, idcg, adcg


def list_grad(s, take, c, idcg, tau):
    """dl/ds of one valid list, 0 for the rows that do not take part"""
    n = s.size
    g = np.zeros(n)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, n, CHUNK):
            b = min(n, a + CHUNK)
            _, dsg = _sigmoid_block(s, a, b, tau)
            ok = np.broadcast_to(take[None, :], dsg.shape).copy()
            ok[np.arange(b - a), np.arange(a, b)] = False
            g[a:b] = np.where(ok, dsg * (c[None, :] - c[a:b, None]), 0.0).sum(1)
        g = g / (tau * idcg)
    return np.where(take, g, 0.0)


def approx_ndcg(scores, labels, groups, mask=None, gain='exp2', temperature=0.1):
    """Result(loss, loss_sum, n_lists, grad of the batch loss per row, approx_rank per row (NaN: does not take part), list_id per row, the rows
    of every list, per list: ADCG, IDCG, valid, loss (0 for an invalid list))."""
    s = np.asarray(scores).reshape(-1).astype(np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    tau = float(temperature)
    B = s.size
    take_all = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    lid = O.list_ids(groups) if B else np.zeros(0, dtype=np.int64)
    lists = O.rows_of_lists(lid)
    n = len(lists)
    R = np.full(B, np.nan)
    grad = np.zeros(B)
    adcg, idcg, lloss = np.zeros(n), np.zeros(n), np.zeros(n)
    valid = np.zeros(n, dtype=bool)
    for g, rows in enumerate(lists):
        take = take_all[rows]
        R[rows], _, _, c, idcg[g], adcg[g] = list_terms(s[rows], y[rows], rows, take, gain, tau)
        valid[g] = idcg[g] > 0
        if not valid[g]:
            continue
        lloss[g] = -adcg[g] / idcg[g]
        grad[rows] = list_grad(s[rows], take, c, idcg[g], tau) if np.isfinite(lloss[g]) else np.where(take, np.nan, 0.0)
    n_lists = int(valid.sum())
    loss_sum = float(lloss[valid].sum()) if n_lists else 0.0
    if n_lists:
        grad = grad / n_lists
    for a in (grad, R, adcg, idcg, valid, lloss):
        a.setflags(write=False)
    return Result(loss_sum / n_lists if n_lists else 0.0, loss_sum, n_lists, grad, R, lid, lists, adcg, idcg, valid, lloss)


def tie_free_batch(sizes, seed):
    """(groups, scores, labels) float32: lists of the given sizes, rows shuffled, scores a permutation of the multiples of 1 / 256 (all
    distinct), labels in {0, 1, 2, 3}.  At temperature 1e-4 every |x| is at least 39, so the soft positions are the hard ones to 1e-16."""
    rng = np.random.default_rng(seed)
    groups = np.repeat(np.arange(len(sizes)), sizes).astype(np.float32)
    rng.shuffle(groups)
    B = groups.size
    scores = ((rng.permutation(B) - B // 2) / 256.0).astype(np.float32)
    labels = rng.integers(0, 4, B).astype(np.float32)
    for a in (groups, scores, labels):
        a.setflags(write=False)
    return groups, scores, labels

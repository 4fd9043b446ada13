"""Per-list fp64 oracle of the in-batch pairwise loss, the layouts that reach every route of the pair walks, and the census that proves it.

Oracle.  Written from the definitions, list by list, so it never forms a B x B matrix (the largest thing it holds is a 512 x n block of one
list) and it reports what a batch-wide oracle cannot: every list's own pair count, loss sum and gradient.  It calls nothing of rec_now_amd
and nothing of the other oracles; tests/test_pair_lists_oracle_cpu.py pins it to tests/_lambda_oracle.py and oracle/dense_ref.py.

  list      the rows that agree in every group tensor; only rows that take part (mask true, or no mask) form pairs and are ranked
  pair      (i, j), i != j, same list, both take part, rule weight w_ij > 0 (w_ij = 1 where label_i > label_j when no rule is given),
            and s_i < s_j under the wrong-order rule
  term      f(u_ij), u_ij = margin - factor (s_i - s_j):  'bpr' softplus at margin 0, 'margin_bpr' softplus, 'hinge' max(u, 0),
            'squared_hinge' max(u, 0)**2
  weight    w_ij * c(main group of i) ** power * lambda_ij, each factor only where it is asked for, all of them constants.  c = the number
            of pairs whose positive row lies in the main group (the first group tensor), ** power formed in float32 as the reference does
            (rec_now/rec_block/pairwise_loss_from_batch.py:130-151: that rounding is part of the contract).
  lambda    |G(y_i) - G(y_j)| |D(r_i) - D(r_j)| / IDCG(list);  r_i = #{ j taking part, j != i : s_j > s_i or (s_j == s_i and j < i) },
            q_i the same on the labels, D(r) = 1 / log2(2 + r) (0 for r >= topn), G(y) = 2**y - 1 or y, IDCG = sum G(y_i) D(q_i)
  loss      sum over the pairs of weight * term, divided by (number of pairs + 1e-10) under reduce_mean
  gradient  d loss / d s_k = factor (sum_i weight_ik f'(u_ik) - sum_j weight_kj f'(u_kj)) / the same divisor

Layouts.  Lists of segment sizes in sorted order (ascending ids), rows shuffled; see LAYOUTS.  Census.  `census(seg_first, B)` restates, in
numpy, which kernel route every sorted row and every block takes (stage_members, PW_LONG and the 64-row phase loop of
csrc/pairwise_walk.hpp and the *_long kernels) and counts the members of each class; CLASSES lists them."""
import collections

import numpy as np
import torch

LEVELS = [0.0, 1.0, 2.0, 3.0]
KINK = 2.0 ** -10
KINDS = ('bpr', 'hinge', 'squared_hinge', 'margin_bpr')
CHUNK = 512


def w_sym(a, b, **k):                            # both directions, tied labels are pairs
    return (a - b).abs() + 0.5


def no_general_route(monkeypatch, M):
    """Patch `pair_indices`, the door to the general route of `M.pairwise_loss`, to raise: a case that must stay fused says so."""
    def refuse(*a, **k):
        raise AssertionError('the general route (pair_indices) was taken')
    monkeypatch.setattr(M, 'pair_indices', refuse)


# ---- lists -------------------------------------------------------------------------------------------------------------------------------
def _as_list(g):
    return list(g) if isinstance(g, (list, tuple)) else [g]


def list_ids(groups):
    """(B,) int64, dense from 0: rows with the same value agree in every group tensor (each tensor is ranked on its own: exact for any dtype)."""
    lid = None
    for t in _as_list(groups):
        _, inv = np.unique(np.asarray(t).reshape(-1), return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        lid = inv if lid is None else lid * (int(inv.max()) + 1 if inv.size else 1) + inv
    if lid.size:
        _, lid = np.unique(lid, return_inverse=True)
    return lid.reshape(-1).astype(np.int64)


def rows_of_lists(lid):
    """the rows of every list, ascending, in the order of the list ids"""
    order = np.argsort(lid, kind='stable')
    n = np.bincount(lid) if lid.size else np.zeros(0, dtype=np.int64)
    return np.split(order, np.cumsum(n)[:-1]) if lid.size else []


# ---- the pair structure of one list ------------------------------------------------------------------------------------------------------
def _rule_weights(rule, yi, yj):
    """(len(yi), len(yj)) fp64 rule weights, 0 where the rule drops the pair (weight <= 0 or NaN)"""
    if rule is None:
        return (yi[:, None] > yj[None, :]).astype(np.float64)
    a = torch.from_numpy(np.array(np.broadcast_to(yi[:, None], (yi.size, yj.size))))
    b = torch.from_numpy(np.array(np.broadcast_to(yj[None, :], (yi.size, yj.size))))
    w = np.asarray(rule(a, b), dtype=np.float64)
    return np.where(w > 0, w, 0.0)


def _block(s, y, take, a, b, rule, wrong):
    """rule weights of the pairs (i, j) with i in [a, b) of one list (local indices), 0 where (i, j) is no pair"""
    w = _rule_weights(rule, y[a:b], y)
    ok = take[a:b, None] & take[None, :]
    ok[np.arange(b - a), np.arange(a, b)] = False
    if wrong:
        ok &= s[a:b, None] < s[None, :]
    return np.where(ok, w, 0.0)


def _f(kind, u):
    """f(u) and f'(u)"""
    if kind == 'hinge':
        return np.maximum(u, 0.0), (u > 0).astype(np.float64)
    if kind == 'squared_hinge':
        h = np.maximum(u, 0.0)
        return h * h, 2.0 * h
    return np.logaddexp(u, 0.0), np.exp(-np.logaddexp(0.0, -u))          # softplus, sigmoid


# ---- NDCG terms ----------------------------------------------------------------------------------------------------------------------------
def _positions(v, rows, take):
    """#{ j taking part, j != i : v_j > v_i or (v_j == v_i and row_j < row_i) } for the rows that take part, -1 for the others"""
    n = v.size
    out = np.full(n, -1, dtype=np.int64)
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        before = (v[None, :] > v[a:b, None]) | ((v[None, :] == v[a:b, None]) & (rows[None, :] < rows[a:b, None]))
        before &= take[None, :]
        before[np.arange(b - a), np.arange(a, b)] = False
        out[a:b] = before.sum(1)
    return np.where(take, out, -1)


def discount(r, topn=None):
    r = np.asarray(r, dtype=np.float64)
    d = 1.0 / np.log2(2.0 + np.maximum(r, 0.0))
    return d if topn is None else np.where(r >= topn, 0.0, d)


def gain_of(y, gain):
    y = np.asarray(y, dtype=np.float64)
    return np.exp2(y) - 1.0 if gain == 'exp2' else y


Terms = collections.namedtuple('Terms', ['rank', 'discount', 'gain', 'inv_idcg', 'list_id', 'dcg', 'idcg', 'ndcg_mean', 'n_lists'])


def rank_terms(scores, labels, groups, mask=None, gain='exp2', topn=None):
    """Per row: position by score (-1 for a row that does not take part), D(position) and G(label) (0 for such a row), 1 / IDCG of the row's
    list (0 where IDCG is not positive), the row's list; per list: DCG, IDCG; the mean of DCG / IDCG over the lists with IDCG > 0 and their number."""
    s = np.asarray(scores).reshape(-1).astype(np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    B = s.size
    take_all = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    lid = list_ids(groups) if B else np.zeros(0, dtype=np.int64)
    lists = rows_of_lists(lid)
    rank = np.full(B, -1, dtype=np.int64)
    disc, gn, inv = np.zeros(B), np.zeros(B), np.zeros(B)
    dcg, idcg = np.zeros(len(lists)), np.zeros(len(lists))
    for g, rows in enumerate(lists):
        take = take_all[rows]
        r = _positions(s[rows], rows, take)
        q = _positions(y[rows], rows, take)
        G = np.where(take, gain_of(y[rows], gain), 0.0)
        D = np.where(take, discount(r, topn), 0.0)
        Dq = np.where(take, discount(q, topn), 0.0)
        rank[rows], disc[rows], gn[rows] = r, D, G
        dcg[g], idcg[g] = (G * D).sum(), (G * Dq).sum()
        inv[rows] = 1.0 / idcg[g] if idcg[g] > 0 else 0.0
    good = idcg > 0
    mean = float((dcg[good] / idcg[good]).mean()) if good.any() else 0.0
    return Terms(rank, disc, gn, inv, lid, dcg, idcg, mean, int(good.sum()))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
Structure = collections.namedtuple('Structure', ['list_id', 'lists', 'cnt_row', 'cnt_list', 'cnt_main', 'main_of_list', 'n_pair'])
ListResult = collections.namedtuple('ListResult', ['rows', 'n_pair', 'loss_sum'])
Result = collections.namedtuple('Result', ['loss', 'n_pair', 'grad', 'lists', 'cnt_row'])


def structure(scores, labels, groups, rule=None, wrong=False, mask=None):
    """Which pairs exist: per row the number of pairs the row is the positive of, per list and per main group their sums.  It does not depend on
    the loss, the occurrence power or the NDCG weight, so one structure serves every case of a (batch, rule, wrong-order, mask)."""
    s = np.asarray(scores).reshape(-1).astype(np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    B = s.size
    take_all = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    lid = list_ids(groups)
    main = list_ids(_as_list(groups)[0])
    lists = rows_of_lists(lid)
    cnt_row = np.zeros(B, dtype=np.int64)
    for rows in lists:
        sl, yl, take = s[rows], y[rows], take_all[rows]
        for a in range(0, rows.size, CHUNK):
            b = min(rows.size, a + CHUNK)
            cnt_row[rows[a:b]] = (_block(sl, yl, take, a, b, rule, wrong) > 0).sum(1)
    cnt_list = np.array([int(cnt_row[rows].sum()) for rows in lists], dtype=np.int64)
    cnt_main = np.bincount(main, weights=cnt_row, minlength=1).astype(np.int64) if B else np.zeros(1, dtype=np.int64)
    main_of_list = np.array([int(main[rows[0]]) for rows in lists], dtype=np.int64)
    for a in (cnt_row, cnt_list, cnt_main, main_of_list):
        a.setflags(write=False)
    return Structure(lid, lists, cnt_row, cnt_list, cnt_main, main_of_list, int(cnt_row.sum()))


def pairwise_loss(scores, labels, groups, kind='bpr', margin=0.0, factor=1.0, reduce_mean=True, rule=None, wrong=False, power=0.0, mask=None,
                  lam=None, pairs=None):
    """Result(loss, number of pairs, gradient per row, per list (rows, pair count, loss sum), per row the number of pairs it is the positive
    of).  rule: None (label_i > label_j, weight 1) or a weight function of two label tensors; lam: None or (gain, topn); pairs: the
    `structure(...)` of the same scores, labels, groups, rule, wrong-order rule and mask, when the caller has it already."""
    assert kind in KINDS
    s = np.asarray(scores).reshape(-1).astype(np.float64)
    y = np.asarray(labels).reshape(-1).astype(np.float64)
    B = s.size
    take_all = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    st = pairs if pairs is not None else structure(s, y, groups, rule, wrong, mask)
    m_eff = 0.0 if kind == 'bpr' else float(margin)
    occ = np.ones(st.cnt_main.size)
    if power != 0.0:
        c32 = torch.from_numpy(st.cnt_main.astype(np.float32))
        p32 = (c32 if power == 1.0 else torch.pow(c32, power)).numpy().astype(np.float64)          # float32, as the reference forms it
        occ = np.where(st.cnt_main > 0, p32, 1.0)                                                 # a main group without pairs has no weight to use
    terms = rank_terms(s, y, groups, mask, lam[0], lam[1]) if lam is not None else None
    denom = (st.n_pair + 1e-10) if reduce_mean else 1.0
    grad = np.zeros(B)
    per_list = []
    total = 0.0
    for g, rows in enumerate(st.lists):
        if st.cnt_list[g] == 0:
            per_list.append(ListResult(rows, 0, 0.0))
            continue
        sl, yl, take = s[rows], y[rows], take_all[rows]
        n = rows.size
        col, row, lsum = np.zeros(n), np.zeros(n), 0.0
        for a in range(0, n, CHUNK):
            b = min(n, a + CHUNK)
            w = _block(sl, yl, take, a, b, rule, wrong) * occ[st.main_of_list[g]]
            if terms is not None:
                G, D = terms.gain[rows], terms.discount[rows]
                w = w * (np.abs(G[a:b, None] - G[None, :]) * np.abs(D[a:b, None] - D[None, :]) * terms.inv_idcg[rows[0]])
            f, df = _f(kind, m_eff - factor * (sl[a:b, None] - sl[None, :]))
            lsum += float((w * f).sum())
            wd = w * df
            row[a:b] = wd.sum(1)
            col += wd.sum(0)
        grad[rows] = factor * (col - row) / denom
        per_list.append(ListResult(rows, int(st.cnt_list[g]), lsum))
        total += lsum
    grad.setflags(write=False)
    return Result(total / denom, st.n_pair, grad, per_list, st.cnt_row)


def assert_off_the_kink(groups, scores, margin, factor):
    """From the fp64 values alone: no two rows of one list (equal scores included) have |margin - factor (s_i - s_j)| below 2**-10."""
    s64 = np.asarray(scores).reshape(-1).astype(np.float64)
    for rows in rows_of_lists(list_ids(groups)):
        if rows.size < 2:
            continue
        v = np.unique(s64[rows])
        assert np.abs(margin - factor * (v[:, None] - v[None, :])).min() >= KINK


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
# Segment sizes in sorted order.  Offsets (the sorted position a segment starts at) are in the comments; T = the 256-row blocks of the
# thread-per-row kernels, W = the 64-row blocks of the wave-per-row kernels.
LAYOUTS = {
    # T block 7 (rows 1792..2047) begins in the 1900 and ends in the 12: a range of 2049 members, NOT staged, with the short 100 / 37 / 12 in it.
    # 513 starts at 2304 = 9 * 256, 600 at 2880 = 45 * 64 (no multiple of 256).  W blocks 29, 44 and 54: (long, short).  B = 3513.
    'r2049': [1900, 100, 37, 12, 200, 55, 513, 1, 2, 60, 600, 33],
    # T block 7 begins in the 1900 and ends with the 11: a range of exactly 2048 members, still staged.  W block 42 (rows 2688..2751): (short,
    # long); T block 10 (2560..2815) runs from the 512 into the 2100 (global) and T block 18 from the 2100 to the end: ranges of 2742 and
    # 2143 members, not staged, so the last 3 rows of the 512, the 130, the 3 and the 40 walk global memory.
    # B = 4836.  One row has the label 7 (outside the table's values) and is masked out.
    'r2048': [1900, 100, 37, 11, 1, 2, 512, 130, 2100, 3, 40],
    # W block 8 (512..575): (staged, global); 40 (2560..2623): (global, staged); 72 (4608..4671): (staged, staged); 81 (5184..5247): (long,
    # short: the 512); 89 (5696..5759): (short, long) over the 2 and the 1; the 700 ends the batch at B = 6425 = 100 * 64 + 25.
    'chain': [513, 2049, 2048, 600, 512, 2, 1, 700],
}
_SEEDS = {'r2049': 41, 'r2048': 42, 'chain': 43}
UNKNOWN_LABEL = 7.0
_BATCHES = {}


def layout(name):
    """(groups, scores, labels, mask) as read-only numpy: ascending float32 ids with the sizes of LAYOUTS[name], rows shuffled; scores =
    round(N(0, 1) * 256) / 256 (long lists are full of ties), labels in {0, 1, 2, 3}, the mask keeps ~80 % of the rows."""
    if name in _BATCHES:
        return _BATCHES[name]
    rng = np.random.default_rng(_SEEDS[name])
    sizes = LAYOUTS[name]
    groups = np.repeat(np.arange(len(sizes)), sizes).astype(np.float32)
    rng.shuffle(groups)
    B = groups.size
    scores = (np.round(rng.normal(size=B) * 256) / 256).astype(np.float32)
    labels = rng.integers(0, 4, B).astype(np.float32)
    mask = rng.random(B) < 0.8
    if name == 'r2048':
        row = int(np.flatnonzero(groups == 1)[5])
        labels[row] = UNKNOWN_LABEL
        mask[row] = False
    for a in (groups, scores, labels, mask):
        a.setflags(write=False)
    _BATCHES[name] = (groups, scores, labels, mask)
    return _BATCHES[name]


def second_groups(B):
    g2 = np.random.default_rng(78).integers(0, 3, B).astype(np.float32)
    g2.setflags(write=False)
    return g2


# ---- census --------------------------------------------------------------------------------------------------------------------------------
PW_LONG, PW_STAGE, T_ROWS, W_ROWS = 512, 2048, 256, 64        # csrc/pairwise_walk.hpp; the block sizes of the two kernel shapes

CLASSES = (
    't_lds',              # sorted rows of short segments whose 256-row block is staged: a thread per row, members from LDS
    't_global',           # ... whose 256-row block is not staged: a thread per row, members from global memory
    't_range_2048',       # 256-row blocks with a short row whose member range is exactly PW_STAGE (still staged)
    't_range_2049',       # ... exactly PW_STAGE + 1 (the first range that is not)
    'w_lds',              # segments of PW_LONG + 1 .. PW_STAGE rows: a wave per row, members from LDS
    'w_global',           # segments of more than PW_STAGE rows: a wave per row, members from global memory
    'size_1', 'size_2', 'size_512', 'size_513', 'size_2048', 'size_2049',
    'w64_staged_staged',  # 64-row blocks whose first and last row lie in two different segments of these kinds (phase 0, phase 1)
    'w64_staged_global',
    'w64_global_staged',
    'w64_short_long',
    'w64_long_short',
    'long_last',          # the last segment is long: its final 64-row block is cut off at B - 1
    'long_on_64',         # long segments that start on a multiple of 64 which is no multiple of 256 (and not at 0)
    'long_on_256',        # long segments that start on a multiple of 256 (not at 0)
)


def trim_seg_first(seg_first, B):
    """the first n_seg + 1 entries of a seg_first array of B + 1 entries (those behind seg_first[n_seg] == B are not written)"""
    sf = np.asarray(seg_first).astype(np.int64).reshape(-1)
    if B == 0:
        return sf[:1]
    end = int(np.flatnonzero(sf[1:] == B)[0]) + 1
    return sf[:end + 1]


def census(seg_first, B):
    """{class: how many rows / blocks / segments are in it} for the segments [seg_first[g], seg_first[g + 1]) of a batch of B sorted rows."""
    sf = trim_seg_first(seg_first, B)
    assert sf[0] == 0 and sf[-1] == B and (np.diff(sf) > 0).all()
    size = np.diff(sf)
    is_long = size > PW_LONG
    kind = np.where(is_long, np.where(size <= PW_STAGE, 1, 2), 0)          # 0 short, 1 long and staged, 2 long from global memory
    seg_of = np.searchsorted(sf, np.arange(B), side='right') - 1
    out = dict.fromkeys(CLASSES, 0)
    for k0 in range(0, B, T_ROWS):                                          # stage_members: one decision per 256-row block
        k1 = min(B, k0 + T_ROWS) - 1
        span = int(sf[seg_of[k1] + 1] - sf[seg_of[k0]])
        short_rows = int((~is_long[seg_of[k0:k1 + 1]]).sum())
        out['t_lds' if span <= PW_STAGE else 't_global'] += short_rows
        if short_rows and span == PW_STAGE:
            out['t_range_2048'] += 1
        if short_rows and span == PW_STAGE + 1:
            out['t_range_2049'] += 1
    out['w_lds'] = int((kind == 1).sum())
    out['w_global'] = int((kind == 2).sum())
    for n in (1, 2, 512, 513, 2048, 2049):
        out['size_%d' % n] = int((size == n).sum())
    names = {(1, 1): 'w64_staged_staged', (1, 2): 'w64_staged_global', (2, 1): 'w64_global_staged'}
    for k0 in range(0, B, W_ROWS):                                          # the phase loop: the segments of the first and the last row
        kl = min(B, k0 + W_ROWS) - 1
        g0, g1 = seg_of[k0], seg_of[kl]
        if g0 == g1:
            continue
        a, b = int(kind[g0]), int(kind[g1])
        if a and b:
            if (a, b) in names:
                out[names[(a, b)]] += 1
        elif b:
            out['w64_short_long'] += 1
        elif a:
            out['w64_long_short'] += 1
    out['long_last'] = int(is_long[-1]) if size.size else 0
    start = sf[:-1]
    out['long_on_64'] = int((is_long & (start > 0) & (start % 64 == 0) & (start % 256 != 0)).sum())
    out['long_on_256'] = int((is_long & (start > 0) & (start % 256 == 0)).sum())
    return out

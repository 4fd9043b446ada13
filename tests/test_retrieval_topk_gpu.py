"""GPU: in_batch_top_k (recnow_ibs_topk, MODE 4 of csrc/in_batch_softmax.hip) against the fp64 per-candidate oracle
tests/_retrieval_topk_oracle.py.

Exact regime (integer entries in [-4, 4], temperature 0.5 or 2, log_q in multiples of 1/8: every logit is exact in fp32, ties are
frequent): scores, indices and n_candidates equal the oracle, the fill included, no tolerance.  Float regime (the inputs of the loss's
tests): no tolerance beyond the project's per-logit 1e-6 -- every returned score within 1e-6 max(1, |s*|) of the fp64 logit AT THE RETURNED
INDEX, the returned fp32 scores in the total order, and every candidate left out at most 2e-6 max(1, |s*_j|, |last|) above the last kept
score (one per-logit bound for each of the two logits compared); no row left out (tests/test_retrieval_topk_cpu.py holds the fp32 torch
composition to the same contract).  Shapes (B, N, D) come from recnow_ibs_tile."""
import numpy as np
import pytest
import torch

import _in_batch_softmax_extra_oracle as X
import _retrieval_ranks_oracle as K
import _retrieval_topk_oracle as O
from rec_now_amd import _lib

pytestmark = pytest.mark.gpu
R, T, G = (_lib.load().recnow_ibs_tile(w) for w in range(3))
assert (R, T) == (K.R, K.T)
XKW = ('extra_item_ids', 'extra_log_q', 'extra_mask')
INF = float('inf')


def _mod():
    from rec_now_amd.rec_block import retrieval_topk as M
    return M


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kw(case, dev):
    kw = dict(item_ids=_t(case['item_ids'], dev), log_q=_t(case['log_q'], dev), temperature=case['temperature'], mask=_t(case['mask'], dev))
    kw.update({k: _t(case[k], dev) for k in XKW})
    return kw


def _run(case, dev, k, in_batch=True, q=None, v=None, x=None, **over):
    """InBatchTopK of one case; q / v / x: ready-made device tensors instead of the case's."""
    q = _t(case['query'], dev) if q is None else q
    v = _t(case['item'], dev) if v is None else v
    x = _t(case.get('extra_item'), dev) if x is None else x
    kw = _kw(case, dev)
    kw.update(over)
    r = _mod().in_batch_top_k(q, v, k=k, extra_item=x, in_batch_candidates=in_batch, **kw)
    B = q.shape[0]
    assert r.scores.shape == (B, k) and r.scores.dtype == torch.float32 and r.indices.shape == (B, k) and r.indices.dtype == torch.int64
    assert r.n_candidates.shape == (B,) and r.n_candidates.dtype == torch.int64 and not any(t.requires_grad for t in r)
    return r


def _np(r):
    return r.scores.cpu().numpy(), r.indices.cpu().numpy(), r.n_candidates.cpu().numpy()


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _exactly(got, want, what=''):
    """Scores, indices and candidate counts equal to the oracle's, the fill and the rows that do not take part included."""
    (s, i, n), (ws, wi, wn) = _np(got), want
    bad = np.argwhere(i != wi)
    assert bad.size == 0, '%s: row %d slot %d holds index %d, the oracle %d' % (what, bad[0][0], bad[0][1], i[tuple(bad[0])], wi[tuple(bad[0])])
    assert np.array_equal(s.astype(np.float64), ws, equal_nan=True), what
    assert np.array_equal(n, wn), what


def _census():
    lib = _lib.load()
    return {(w, vec): lib.recnow_ibs_topk_launches(w, vec) for w in range(4) for vec in (0, 1)}


def _old_census():
    lib = _lib.load()
    return [lib.recnow_ibs_extra_launches(w, vec) for w in range(4) for vec in (0, 1)] + \
           [lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)] + \
           [lib.recnow_ibs_launches(o, vec) for o in (0, 1, 2, 4, 5, 6) for vec in (0, 1)]


def _copy(case):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}


# ---- 1. the exact regime ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('config', K.CONFIGS)
@pytest.mark.parametrize('B,N,D', K.EXACT_SHAPES)
def test_exact_inputs_give_the_oracle_lists_exactly(dev, B, N, D, config, in_batch):
    case, ref, rows = O.exact_sorted(B, N, D, config, in_batch)
    if config == 'plain' and in_batch and B >= T:
        assert any(len({s for _, s in row}) < len(row) for row in ref['cands'])        # ties are frequent here
    for k in O.KS:
        _exactly(_run(case, dev, k, in_batch), O.topk_of_sorted(rows, k), 'K = %d' % k)


# ---- 2. the float regime ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('config', K.CONFIGS)
@pytest.mark.parametrize('B,N,D', K.SHAPES)
def test_float_inputs_hold_the_per_logit_bound_and_the_total_order(dev, B, N, D, config, in_batch):
    case, ref = K.float_ref(B, N, D, config, in_batch)
    for k in O.KS:
        worst = O.check_float_regime(*_np(_run(case, dev, k, in_batch)), ref, k)
        print('K = %3d: worst score error %.3f of the bound, worst excluded candidate %.3f of its bound' % ((k,) + worst))


# ---- 3. agreement with in_batch_ranks, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('regime', ['exact', 'float'])
@pytest.mark.parametrize('B,N,D,config', [(197, 129, 64, 'all'), (129, 97, 128, 'mask'), (64, 33, 33, 'plain'), (32, 130, 16, 'log_q')])
def test_the_list_agrees_with_the_counts_of_in_batch_ranks(dev, B, N, D, config, regime, in_batch):
    from rec_now_amd.rec_block import retrieval_metrics as RM
    case = (K.exact_ref if regime == 'exact' else K.float_ref)(B, N, D, config, in_batch)[0]
    q, v, x = (_t(case[k], dev) for k in ('query', 'item', 'extra_item'))
    ranks = RM.in_batch_ranks(q, v, extra_item=x, in_batch_candidates=in_batch, **_kw(case, dev))
    pos = ranks.row_pos_logit[:, None]
    for k in (1, 5, 33, 128):
        got = _run(case, dev, k, in_batch)
        assert torch.equal(got.n_candidates, ranks.n_candidates)
        kk = torch.full_like(ranks.n_greater, k)
        above = ((got.indices >= 0) & ~(got.scores <= pos)).sum(1)
        assert torch.equal(above, torch.minimum(kk, ranks.n_greater))
        equal = ((got.indices >= 0) & (got.scores == pos)).sum(1)
        assert torch.equal(equal, torch.minimum(kk - torch.minimum(kk, ranks.n_greater), ranks.n_equal))
    assert regime == 'float' or not in_batch or ranks.n_equal.any()


# ---- 4. the order of arrival ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['ascending', 'descending', 'constant'])
def test_every_candidate_displaces_one_or_none_does(dev, order):
    """query = e_0 and column 0 of the candidates a ramp over the streamed position: ascending, every candidate past the first K displaces
    the worst kept one, in both half-waves of a row within one tile; descending, none does; constant, the index alone decides."""
    B, N, D = R + T + 1, 2 * T + 7, 4
    ramp = {'ascending': np.arange(B + N), 'descending': -np.arange(B + N), 'constant': np.zeros(B + N)}[order].astype(np.float32)
    rows = np.zeros((B + N, D), dtype=np.float32)
    rows[:, 0] = ramp
    rows[:, 1] = 1.0
    query = np.zeros((B, D), dtype=np.float32)
    query[:, 0] = 1.0
    query[:, 1] = np.arange(B) % 3                             # rows differ, their orders do not
    case = dict(query=query, item=rows[:B], extra_item=rows[B:], item_ids=None, log_q=None, mask=None, temperature=1.0,
                extra_item_ids=None, extra_log_q=None, extra_mask=None)
    for in_batch in (True, False):
        ref = K.ranks_of(case, in_batch_candidates=in_batch)
        for k in (5, 32, 128):
            got = _run(case, dev, k, in_batch)
            _exactly(got, O.topk_oracle(ref, k), '%s K = %d' % (order, k))
            first = got.indices[0, 0].item()
            assert first == {'ascending': B + N - 1, 'descending': 1 if in_batch else B, 'constant': 1 if in_batch else B}[order]


# ---- 5. the prefix property -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('regime', ['exact', 'float'])
def test_a_shorter_list_is_the_head_of_a_longer_one_bit_for_bit(dev, regime, in_batch):
    case = (K.exact_ref if regime == 'exact' else K.float_ref)(197, 129, 64, 'all', in_batch)[0]
    full = _run(case, dev, 128, in_batch)
    for k in (5, 33):
        got = _run(case, dev, k, in_batch)
        assert torch.equal(_bits(got.scores), _bits(full.scores[:, :k])) and torch.equal(got.indices, full.indices[:, :k])
        assert torch.equal(got.n_candidates, full.n_candidates)
    assert (full.indices >= 0).any()


# ---- 6. bit-identical copies ------------------------------------------------------------------------------------------------------------------
def _duplicates_case(config):
    """Bit-identical copies of one candidate row (and of its log_q), scaled to stand above everything else: at EVERY position of streamed
    tile 1, at two places of the last, ragged batch tile, and at five places of the extras, the last, ragged extras tile among them."""
    B, N, D = R + T + 5, T + 7, 16
    case = _copy(K.make_extra_case(B, N, D, config, R, T, seed=3))
    case['mask'] = case['extra_mask'] = None
    batch = sorted(set(range(T, 2 * T)) | {B - 3, B - 1})
    extras = [0, 5, T - 1, T, N - 1]
    case['query'][:, 0] = 3.0                                # the copies score 12 + ...: above every other candidate of every row
    row = case['item'][T].copy()
    row[0] = 4.0
    case['item'][batch] = row
    case['extra_item'][extras] = row
    if case['log_q'] is not None:
        case['log_q'][batch] = case['log_q'][T]
        case['extra_log_q'][extras] = case['log_q'][T]
    return case, batch, extras


@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('config', ['plain', 'log_q'])
def test_bit_identical_copies_come_in_index_order_or_are_removed_by_id(dev, config, in_batch):
    case, batch, extras = _duplicates_case(config)
    B, N = case['query'].shape[0], case['extra_item'].shape[0]
    i0, other = 3, R + 2                                       # two rows that are no copies: wave 0 and the second workgroup
    copies = ([j for j in batch] if in_batch else []) + [B + e for e in extras]
    for k in (5, len(copies), 128):
        got = _run(case, dev, k, in_batch)
        s, i, n = _np(got)
        for r in (i0, other):
            head = min(k, len(copies))
            assert i[r, :head].tolist() == copies[:head], 'row %d: the copies do not come in index order' % r
            assert len(set(s[r, :head].view(np.int32).tolist())) == 1          # one score, bit for bit, wherever the copy stood
        O.check_float_regime(s, i, n, K.ranks_of(case, in_batch_candidates=in_batch), k)
    # with ids: the copies carry row i0's id and are removed, for row i0 alone
    ids, xids = np.arange(B, dtype=np.int64) * 3 + 1, np.arange(N, dtype=np.int64) * 3 + 2
    ids[batch], xids[extras] = ids[i0], ids[i0]
    got = _run(case, dev, 128, in_batch, item_ids=_t(ids, dev), extra_item_ids=_t(xids, dev))
    s, i, n = _np(got)
    assert not np.isin(i[i0], copies).any() and n[i0] == (B - 1 if in_batch else 0) + N - len(copies)
    assert i[other, :len(copies)].tolist() == copies and n[other] == (B - 1 if in_batch else 0) + N
    O.check_float_regime(s, i, n, K.ranks_of(case, in_batch_candidates=in_batch, item_ids=ids, extra_item_ids=xids), 128)


# ---- 7. special logits ----------------------------------------------------------------------------------------------------------------------
def test_nan_stands_first_and_infinite_candidates_keep_their_indices(dev):
    case, _ = K.exact_ref(197, 129, 64, 'mask')
    c = _copy(case)
    B, N = 197, 129
    xs = np.flatnonzero(case['extra_mask'])
    k_nan, k_pinf, k_ninf = xs[-1], xs[3], xs[len(xs) // 2]
    c['extra_item'][k_nan, 63] = np.nan                    # an extra every taking-part row sees
    c['log_q'] = np.zeros(B, dtype=np.float32)
    c['extra_log_q'] = np.zeros(N, dtype=np.float32)
    c['extra_log_q'][k_pinf] = -INF                        # a logit of +inf
    c['extra_log_q'][k_ninf] = INF                         # and one of -inf: a candidate still
    i0 = np.flatnonzero(case['mask'])[5]
    c['log_q'][i0] = INF                                   # a -inf batch candidate too (and row i0's positive)
    for in_batch in (True, False):
        ref = K.ranks_of(c, in_batch_candidates=in_batch)
        big = int(ref['n_candidates'].max())
        assert big > 128 or not in_batch
        for k in (1, 5, 128):
            got = _run(c, dev, k, in_batch)
            _exactly(got, O.topk_oracle(ref, k), 'K = %d' % k)
            s, i, n = _np(got)
            on = ref['on']
            assert (i[on, 0] == B + k_nan).all() and np.isnan(s[on, 0]).all()
            if k >= 5:
                assert (i[on, 1] == B + k_pinf).all() and np.isposinf(s[on, 1]).all()
    # few enough candidates that the -inf ones are kept: they carry their indices and stand before the fill
    small = _copy(c)
    keep = np.zeros(N, dtype=bool)
    keep[[k_nan, k_pinf, k_ninf, xs[0]]] = True
    small['extra_mask'] = keep
    ref = K.ranks_of(small, in_batch_candidates=False)
    got = _run(small, dev, 8, False)
    _exactly(got, O.topk_oracle(ref, 8))
    s, i, n = _np(got)
    on = ref['on']
    assert (n[on] == 4).all() and (i[on, 3] == B + k_ninf).all() and np.isneginf(s[on, 3]).all() and (i[on, 4:] == -1).all()
    assert (i[on, 0] == B + k_nan).all() and (i[on, 1] == B + k_pinf).all() and (i[on, 2] == B + xs[0]).all()


def test_a_row_with_fewer_than_k_candidates_a_lone_row_and_an_empty_corpus(dev):
    M = _mod()
    q, v = torch.full((1, 7), 0.5, device=dev), torch.full((1, 7), 2.0, device=dev)
    r = M.in_batch_top_k(q, v, k=3)                        # a row that is its own only candidate: all fill
    assert r.scores.tolist() == [[-INF] * 3] and r.indices.tolist() == [[-1] * 3] and r.n_candidates.tolist() == [0]
    r = M.in_batch_top_k(q, v, k=128, extra_item=torch.zeros((0, 7), device=dev), in_batch_candidates=False)      # an empty corpus
    assert torch.isneginf(r.scores).all() and (r.indices == -1).all() and r.n_candidates.tolist() == [0] and r.scores.shape == (1, 128)
    x = torch.tensor([[1.0] * 7, [3.0] * 7], device=dev)   # a lone row with two extras
    for in_batch in (True, False):
        r = M.in_batch_top_k(q, v, k=4, extra_item=x, in_batch_candidates=in_batch)
        assert r.scores.tolist() == [[10.5, 3.5, -INF, -INF]] and r.indices.tolist() == [[2, 1, -1, -1]] and r.n_candidates.tolist() == [2]
    case, ref = K.exact_ref(33, 32, 8, 'all')              # fewer than K candidates in every row
    assert 0 < ref['n_candidates'].max() < 128
    _exactly(_run(case, dev, 128), O.topk_oracle(ref, 128))


@pytest.mark.parametrize('B,N', [(1, 3), (R + 3, T + 7)])
def test_extras_that_are_all_hits_or_masked_are_nobodys_candidates(dev, B, N):
    case = K.exact_case(B, N, 33, 'log_q')
    case['extra_mask'] = np.zeros(N, dtype=bool)                          # all masked: the batch columns are left
    _exactly(_run(case, dev, 33), O.topk_oracle(K.ranks_of(case), 33), 'masked')
    case['item_ids'] = np.full(B, 11, dtype=np.int64)                     # every other row is a hit; every second extra too, the others masked
    case['extra_item_ids'] = np.where(np.arange(N) % 2 == 0, 11, 12).astype(np.int64)
    case['extra_mask'] = np.arange(N) % 2 == 0
    for in_batch in (True, False):
        got = _run(case, dev, 5, in_batch)
        assert (got.indices == -1).all() and torch.isneginf(got.scores).all() and not got.n_candidates.any()
        _exactly(got, O.topk_oracle(K.ranks_of(case, in_batch_candidates=in_batch), 5), 'hits')


# ---- 8. masked inputs -----------------------------------------------------------------------------------------------------------------------
def test_masked_rows_and_masked_extras_full_of_nan_and_inf_touch_no_bit(dev):
    B, N, D = 129, 97, 128
    case, _ = K.float_ref(B, N, D, 'all')
    off, xoff = ~case['mask'], ~case['extra_mask']
    fill = np.where(np.arange(D) % 3 == 0, np.nan, np.where(np.arange(D) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    for in_batch in (True, False):
        for k in (5, 128):
            outs = []
            for bad in (False, True):
                c = _copy(case)
                for key, rows in (('query', off), ('item', off), ('extra_item', xoff)):
                    c[key][rows] = fill if bad else 0.25
                c['log_q'][off] = np.nan if bad else 0.0
                c['extra_log_q'][xoff] = -np.inf if bad else 0.0
                outs.append(_run(c, dev, k, in_batch))
            assert off.sum() > T and xoff.sum() > T and _same(outs[0], outs[1])
            gone = torch.from_numpy(off).to(dev)
            assert (outs[1].indices[gone] == -1).all() and torch.isneginf(outs[1].scores[gone]).all() and not outs[1].n_candidates[gone].any()
            assert torch.isfinite(outs[1].scores[~gone][:, 0]).all()


# ---- 9. magnitude 100 -----------------------------------------------------------------------------------------------------------------------
def test_logits_of_magnitude_100_with_the_greatest_candidate_at_every_tile_position(dev):
    """Entries +-1/4 in D = 16, temperature 0.01: every logit is a multiple of 12.5, exact in fp32.  query_i = extra_c(i) with c a bijection:
    row i's greatest candidate (100) stands at extra c(i), which visits every position of an extras tile and the ragged last tile."""
    B = N = 2 * T + 5
    rng = np.random.default_rng(5)
    rows = (rng.integers(0, 2, (B + N, 16)) * 2 - 1).astype(np.float32) / 4
    assert len({r.tobytes() for r in rows}) == B + N
    c = (np.arange(B) * 5 + 3) % N
    case = dict(query=rows[B:][c].copy(), item=rows[:B], extra_item=rows[B:], item_ids=None, log_q=None, mask=None, temperature=0.01,
                extra_item_ids=None, extra_log_q=None, extra_mask=None)
    assert set(c % T) == set(range(T)) and (c >= 2 * T).any()
    for in_batch in (True, False):
        ref = K.ranks_of(case, in_batch_candidates=in_batch)
        for k in (1, 33):
            got = _run(case, dev, k, in_batch)
            _exactly(got, O.topk_oracle(ref, k))
            assert got.indices[:, 0].tolist() == (B + c).tolist() and (got.scores[:, 0] == 100.0).all()


# ---- 10. corpus mode ------------------------------------------------------------------------------------------------------------------------
def test_the_corpus_alone_leaves_the_item_segment_unwalked_and_is_the_masked_restatement(dev):
    B, N, D = 33, 32, 8
    for config in ('plain', 'all'):
        case, _ = K.exact_ref(B, N, D, config)
        before = _census()
        got = _np(_run(case, dev, 7, False))
        now = _census()
        assert now[(3, 0)] == before[(3, 0)] + 1 and now[(3, 1)] == before[(3, 1)] and now[(1, 1)] == before[(1, 1)] + 1
        on = np.ones(B, dtype=bool) if case['mask'] is None else case['mask']
        for i in range(B):                                 # row i with every other batch row masked out of the candidate set
            m = np.zeros(B, dtype=bool)
            m[i] = on[i]
            one = _np(_run(case, dev, 7, True, mask=_t(m, dev)))
            assert all(np.array_equal(a[i], b[i]) for a, b in zip(one, got))
        assert _census()[(3, 1)] == now[(3, 1)] + B
        assert (got[1][got[1] >= 0] >= B).all()            # corpus indices still address cat(item, extra_item)


# ---- 11. views and the census -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,D', [(197, 129, 64), (64, 33, 33)])
def test_row_strided_and_offset_views_give_the_aligned_bits(dev, B, N, D):
    case, _ = K.float_ref(B, N, D, 'all')
    want = _run(case, dev, 33)
    for col in (4, 1):                                 # a column slice of a wider tower output; col 1: the storage is off by one float
        wide = [torch.full((n, D + 12), 7.0, device=dev) for n in (B, B, N)]
        for w, key in zip(wide, ('query', 'item', 'extra_item')):
            w[:, col:col + D] = _t(case[key], dev)
        q, v, x = (w[:, col:col + D] for w in wide)
        before = _census()
        got = _run(case, dev, 33, q=q, v=v, x=x)
        now = _census()
        assert _same(want, got)
        if D == 64:                                    # the views themselves reached the kernel: guarded accesses for col 1
            vec = 1 if col == 4 else 0
            assert all(now[(w, vec)] == before[(w, vec)] + 1 and now[(w, 1 - vec)] == before[(w, 1 - vec)] for w in (0, 1, 2))
    xt = _t(case['extra_item'].T.copy(), dev).T        # column-major: made contiguous, same bits
    assert _same(want, _run(case, dev, 33, x=xt))


def test_census_every_width_of_every_side_and_the_other_censuses_untouched(dev):
    lib = _lib.load()
    old = _old_census()
    before = _census()
    _run(K.float_ref(65, 1, 64, 'plain')[0], dev, 3)            # 16-byte accesses throughout, the items walked
    _run(K.float_ref(2, 31, 3, 'plain')[0], dev, 3, False)      # none, the items left out
    now = _census()
    assert all(now[key] == before[key] + 1 for key in now)
    case = K.float_ref(65, 1, 64, 'plain')[0]                   # no extras: the extras' census does not move
    _mod().in_batch_top_k(_t(case['query'], dev), _t(case['item'], dev), k=3)
    last = _census()
    assert last[(2, 0)] == now[(2, 0)] and last[(2, 1)] == now[(2, 1)] and last[(0, 1)] == now[(0, 1)] + 1 and last[(3, 1)] == now[(3, 1)] + 1
    assert old == _old_census()                                 # top-K launches are in no census of the loss or of the ranks
    assert lib.recnow_ibs_topk_launches(4, 0) < 0 and lib.recnow_ibs_topk_launches(0, 2) < 0 and lib.recnow_ibs_topk_launches(-1, 0) < 0


def test_the_c_entry_honours_the_leading_dimensions_of_its_outputs(dev):
    B, N, D, k = 65, 33, 16, 5
    case = K.exact_case(B, N, D, 'plain')
    q, v, x = (_t(case[key], dev) for key in ('query', 'item', 'extra_item'))
    want = _mod().in_batch_top_k(q, v, k=k, extra_item=x, temperature=case['temperature'])
    scores = torch.full((B, 2 * k), 7.0, device=dev)
    indices = torch.full((B, 2 * k + 3), 7, dtype=torch.int64, device=dev)
    n_cand = torch.zeros(B, dtype=torch.int64, device=dev)
    P = _lib.ptr
    _lib.call('recnow_ibs_topk', P(q), D, P(v), D, None, None, None, B, D, P(x), D, None, None, None, N, 1.0 / case['temperature'], 1, 1, k,
              P(scores), 2 * k, P(indices), 2 * k + 3, P(n_cand), _lib.stream())
    assert torch.equal(_bits(scores[:, :k]), _bits(want.scores)) and torch.equal(indices[:, :k], want.indices)
    assert (scores[:, k:] == 7.0).all() and (indices[:, k:] == 7).all() and torch.equal(n_cand, want.n_candidates)


# ---- 12. repeatability ------------------------------------------------------------------------------------------------------------------------
def test_repeated_runs_and_graph_replay_are_bit_for_bit(dev):
    M = _mod()
    case, _ = K.float_ref(197, 129, 64, 'all')
    assert _same(_run(case, dev, 128), _run(case, dev, 128)) and _same(_run(case, dev, 33, False), _run(case, dev, 33, False))
    q, v, x = (_t(case[k], dev) for k in ('query', 'item', 'extra_item'))
    kw = _kw(case, dev)

    def step():
        return tuple(M.in_batch_top_k(q, v, k=100, extra_item=x, **kw)) + tuple(M.in_batch_top_k(q, v, k=10, extra_item=x, **kw))
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(9)
    for _ in range(2):
        for t in (q, v, x):                                # new contents, same storage
            t.copy_(torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32) * 0.3))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert _same(outs, eager) and (outs[1] >= 0).any() and torch.equal(outs[0][:, :10], outs[3])


# ---- 13. memory -----------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_holds_no_b_by_b_plus_n_matrix(dev):
    """in_batch_top_k at B 1024, N 3072, D 32, K 100: above the inputs, the outputs (K scores and K indices a row, the candidate counts),
    the per-row vectors as the kernel reads them (int64 ids where int32 came in, uint8 masks) and a 64 KB allowance; one (B, B + N) fp32
    matrix would be 16 MB."""
    M = _mod()
    B, N, D, k = 1024, 3072, 32, 100
    gen = torch.Generator(device='cpu').manual_seed(3)
    q, v = ((torch.randn(B, D, generator=gen) * 0.4).to(dev) for _ in range(2))
    x = (torch.randn(N, D, generator=gen) * 0.4).to(dev)
    ids = torch.randint(0, B // 4, (B,), generator=gen, dtype=torch.int32).to(dev)
    xids = torch.randint(0, B // 4, (N,), generator=gen, dtype=torch.int32).to(dev)
    lq, xlq = torch.rand(B, generator=gen).add_(0.05).log_().to(dev), torch.rand(N, generator=gen).add_(0.05).log_().to(dev)
    m, xm = (torch.rand(B, generator=gen) > 0.1).to(dev), (torch.rand(N, generator=gen) > 0.1).to(dev)

    def step():
        return M.in_batch_top_k(q, v, item_ids=ids, log_q=lq, temperature=0.7, mask=m, k=k, extra_item=x, extra_item_ids=xids, extra_log_q=xlq,
                                extra_mask=xm)
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = (12 * k + 8) * B + (8 + 2) * (B + N) + 65536             # outputs; int64 ids, bool and uint8 masks; the allowance
    assert (r.indices[m] >= 0).all() and (r.indices[~m] == -1).all()
    assert rise <= allowed < B * (B + N) * 4 // 8, 'in_batch_top_k rose %d bytes, allowed %d' % (rise, allowed)


# ---- 14. the use itself ---------------------------------------------------------------------------------------------------------------------
def test_mined_hard_negatives_feed_the_loss(dev):
    """Mine the K hardest negatives of a memory bank per row, gather their union into extra_item of in_batch_softmax_loss, and compare with
    the fp64 oracle of that loss on the same gathered rows."""
    from rec_now_amd.rec_block import in_batch_softmax as L
    B, N, D, k = 65, 130, 16, 4
    case = X.make_extra_case(B, N, D, 'log_q', R, T, seed=5)
    q, v, bank = (_t(case[key], dev) for key in ('query', 'item', 'extra_item'))
    lq, blq = _t(case['log_q'], dev), _t(case['extra_log_q'], dev)
    mined = _mod().in_batch_top_k(q, v, log_q=lq, temperature=case['temperature'], k=k, extra_item=bank, extra_log_q=blq,
                                  in_batch_candidates=False)
    assert (mined.indices >= B).all() and (mined.n_candidates == N).all()
    O.check_float_regime(*_np(mined), K.ranks_of(case, in_batch_candidates=False), k)
    pick = torch.unique(mined.indices.reshape(-1) - B)                 # the union of every row's hardest bank entries
    assert k <= pick.numel() < N
    loss = L.in_batch_softmax_loss(q, v, log_q=lq, temperature=case['temperature'], extra_item=bank[pick], extra_log_q=blq[pick])
    rows = pick.cpu().numpy()
    oracle = X.oracle_of(dict(case, extra_item=case['extra_item'][rows], extra_log_q=case['extra_log_q'][rows]))
    assert abs(loss.item() - oracle['loss']) <= 1e-5 * abs(oracle['loss'])                 # the loss's own bound

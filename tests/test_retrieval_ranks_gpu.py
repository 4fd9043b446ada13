"""GPU: in_batch_ranks / in_batch_retrieval_metrics (recnow_ibs_rank, MODE 3 of csrc/in_batch_softmax.hip) against the fp64 per-candidate
oracle tests/_retrieval_ranks_oracle.py.

Exact regime (integer entries in [-4, 4], temperature 0.5 or 2, log_q in multiples of 1/8: every logit is exact in fp32): the three counts
and row_pos_logit equal the oracle, no tolerance.  Float regime (the inputs of the loss's tests): the guard band
  eps_ij = 2e-6 max(1, |s_ij|, |s_ii|)          the project's 1e-6 per-logit bound, once for each of the two logits compared
  G_lo = #{s_ij - s_ii > eps},  G_hi = #{s_ij - s_ii > -eps}  over C'(i);    G_lo <= n_greater  and  n_greater + n_equal <= G_hi
with n_candidates and n_rows exact, row_pos_logit within 1e-6 max(1, |ref|), and no row left out (tests/test_retrieval_ranks_cpu.py holds
the fp32 torch composition to the same band and shows it is narrow).  Shapes (B, N, D) come from recnow_ibs_tile."""
import numpy as np
import pytest
import torch

import _retrieval_ranks_oracle as K
from rec_now_amd import _lib

pytestmark = pytest.mark.gpu
R, T, G = (_lib.load().recnow_ibs_tile(w) for w in range(3))
assert (R, T) == (K.R, K.T)
COUNTS = ('n_greater', 'n_equal', 'n_candidates')
XKW = ('extra_item_ids', 'extra_log_q', 'extra_mask')


def _mod():
    from rec_now_amd.rec_block import retrieval_metrics as M
    return M


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kw(case, dev):
    kw = dict(item_ids=_t(case['item_ids'], dev), log_q=_t(case['log_q'], dev), temperature=case['temperature'], mask=_t(case['mask'], dev))
    kw.update({k: _t(case[k], dev) for k in XKW})
    return kw


def _run(case, dev, in_batch=True, q=None, v=None, x=None, **over):
    """InBatchRanks of one case; q / v / x: ready-made device tensors instead of the case's."""
    q = _t(case['query'], dev) if q is None else q
    v = _t(case['item'], dev) if v is None else v
    x = _t(case['extra_item'], dev) if x is None else x
    kw = _kw(case, dev)
    kw.update(over)
    r = _mod().in_batch_ranks(q, v, extra_item=x, in_batch_candidates=in_batch, **kw)
    B = q.shape[0]
    assert all(t.shape == (B,) and t.dtype == torch.int64 for t in r[:3]) and r.row_pos_logit.shape == (B,)
    assert r.row_pos_logit.dtype == torch.float32 and r.n_rows.dim() == 0 and not any(t.requires_grad for t in r)
    return r


def _np(r):
    return {k: getattr(r, k).cpu().numpy() for k in COUNTS + ('row_pos_logit',)}


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _exactly(got, ref, what=''):
    """Counts and the positive's logit equal to the oracle's, the rows that do not take part included (0, 0, 0, NaN)."""
    g = _np(got)
    for k in COUNTS:
        bad = np.flatnonzero(g[k] != ref[k])
        assert bad.size == 0, '%s %s: row %d has %d, the oracle %d' % (what, k, bad[0], g[k][bad[0]], ref[k][bad[0]])
    assert np.array_equal(g['row_pos_logit'].astype(np.float64), ref['pos'], equal_nan=True), what
    assert got.n_rows.item() == ref['n']


def _census():
    lib = _lib.load()
    return {(w, vec): lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)}


def _old_census():
    lib = _lib.load()
    return [lib.recnow_ibs_extra_launches(w, vec) for w in range(4) for vec in (0, 1)] + \
           [lib.recnow_ibs_launches(o, vec) for o in (0, 1, 2, 4, 5, 6) for vec in (0, 1)]


# ---- 1. the exact regime ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('config', K.CONFIGS)
@pytest.mark.parametrize('B,N,D', K.EXACT_SHAPES)
def test_exact_inputs_give_the_oracle_counts_exactly(dev, B, N, D, config, in_batch):
    case, ref = K.exact_ref(B, N, D, config, in_batch)
    if config == 'plain' and in_batch and B >= T:
        assert ref['n_equal'].any()                        # ties are frequent here
    _exactly(_run(case, dev, in_batch), ref)


# ---- 2. the float regime ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('config', K.CONFIGS)
@pytest.mark.parametrize('B,N,D', K.SHAPES)
def test_float_inputs_stay_inside_the_guard_band(dev, B, N, D, config, in_batch):
    case, ref = K.float_ref(B, N, D, config, in_batch)
    got = _run(case, dev, in_batch)
    g, on = _np(got), ref['on']
    assert np.array_equal(g['n_candidates'], ref['n_candidates']) and got.n_rows.item() == ref['n']
    assert (ref['g_lo'] <= g['n_greater']).all() and (g['n_greater'] + g['n_equal'] <= ref['g_hi']).all()      # every row: none is left out
    assert not g['n_greater'][~on].any() and not g['n_equal'][~on].any() and np.isnan(g['row_pos_logit'][~on]).all()
    if on.any():
        frac = np.abs(g['row_pos_logit'][on] - ref['pos'][on]) / (1e-6 * np.maximum(1.0, np.abs(ref['pos'][on])))
        print('row_pos_logit: worst %.3f of the bound; %d ambiguous rows' % (frac.max(), (ref['g_lo'] != ref['g_hi']).sum()))
        assert frac.max() <= 1.0


# ---- 3. duplicates of the positive ---------------------------------------------------------------------------------------------------------
def _duplicates_case(i0, config):
    """Bit-identical copies of row i0's item (and of its log_q): at EVERY position of the streamed tile 1, at two places of the last,
    ragged batch tile, and at five places of the extras, the last, ragged extras tile among them."""
    B, N, D = R + T + 5, T + 7, 16
    case = K.make_extra_case(B, N, D, config, R, T, seed=3)
    case['mask'] = case['extra_mask'] = None
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    batch = sorted((set(range(T, 2 * T)) | {B - 3, B - 1}) - {i0})
    extras = [0, 5, T - 1, T, N - 1]
    case['item'][batch] = case['item'][i0]
    case['extra_item'][extras] = case['item'][i0]
    if case['log_q'] is not None:
        case['log_q'][batch] = case['log_q'][i0]
        case['extra_log_q'][extras] = case['log_q'][i0]
    return case, batch, extras


@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('i0', [3, T + 6, R + T + 1])     # wave 0 / half 0;  wave 1 / half 1, inside the tile of copies;  the ragged last tile
def test_bit_identical_copies_of_the_positive_are_counted_equal_or_removed_by_id(dev, i0, in_batch):
    for config in ('plain', 'log_q'):
        case, batch, extras = _duplicates_case(i0, config)
        B, N = case['query'].shape[0], case['extra_item'].shape[0]
        copies = len(extras) + (len(batch) if in_batch else 0)
        ref = K.ranks_of(case, in_batch_candidates=in_batch)
        rest = np.setdiff1d(np.arange(B), batch + [i0])    # (a row whose own item is a copy ties with the other copies; no other row ties)
        assert ref['n_equal'][i0] == copies and not ref['n_equal'][rest].any()
        got = _np(_run(case, dev, in_batch))
        assert got['n_equal'][i0] == copies, 'row %d: %d of %d copies counted equal' % (i0, got['n_equal'][i0], copies)
        assert got['n_candidates'][i0] == (B - 1 if in_batch else 0) + N
        assert ref['g_lo'][i0] <= got['n_greater'][i0] and got['n_greater'][i0] + copies <= ref['g_hi'][i0]
        # with ids: the copies carry row i0's id and are removed, for row i0 alone
        ids, xids = np.arange(B, dtype=np.int64) * 3 + 1, np.arange(N, dtype=np.int64) * 3 + 2
        ids[batch], xids[extras] = ids[i0], ids[i0]
        got_ids = _np(_run(case, dev, in_batch, item_ids=_t(ids, dev), extra_item_ids=_t(xids, dev)))
        assert got_ids['n_equal'][i0] == 0 and got_ids['n_candidates'][i0] == got['n_candidates'][i0] - copies
        assert got_ids['n_greater'][i0] == got['n_greater'][i0]
        other = R + 2                                      # a row that is no copy keeps them all as candidates
        assert got_ids['n_candidates'][other] == got['n_candidates'][other] and got_ids['n_greater'][other] == got['n_greater'][other]


# ---- 4. agreement with the loss -------------------------------------------------------------------------------------------------------------
def _terms(case, dev, q=None, v=None, x=None, extras=True):
    from rec_now_amd.rec_block import in_batch_softmax as L
    q = _t(case['query'], dev) if q is None else q
    v = _t(case['item'], dev) if v is None else v
    kw = _kw(case, dev)
    if not extras:
        return L.in_batch_softmax_terms(q, v, **{k: w for k, w in kw.items() if k not in XKW})
    return L.in_batch_softmax_terms(q, v, extra_item=_t(case['extra_item'], dev) if x is None else x, **kw)


@pytest.mark.parametrize('config', ['plain', 'all'])
@pytest.mark.parametrize('B,N,D', [(197, 129, 64), (129, 97, 128), (64, 33, 33)])
def test_row_pos_logit_is_that_of_the_loss_bit_for_bit(dev, B, N, D, config):
    case, _ = K.float_ref(B, N, D, config)
    M = _mod()
    with_x = _terms(case, dev)
    assert torch.equal(_bits(_run(case, dev).row_pos_logit), _bits(with_x.row_pos_logit))
    assert torch.equal(_bits(_run(case, dev, False).row_pos_logit), _bits(with_x.row_pos_logit))      # the corpus alone: the same positive
    kw = {k: w for k, w in _kw(case, dev).items() if k not in XKW}
    square = M.in_batch_ranks(_t(case['query'], dev), _t(case['item'], dev), **kw)                  # the square case: no extras at all
    assert torch.equal(_bits(square.row_pos_logit), _bits(_terms(case, dev, extras=False).row_pos_logit))
    assert torch.isfinite(square.row_pos_logit).sum().item() == square.n_rows.item() > 0


@pytest.mark.parametrize('B,N,D', [(197, 129, 64), (64, 33, 33)])
def test_row_strided_and_offset_views_give_the_aligned_bits_and_the_positive_of_the_loss(dev, B, N, D):
    case, _ = K.float_ref(B, N, D, 'all')
    want = _run(case, dev)
    for col in (4, 1):                                 # a column slice of a wider tower output; col 1: the storage is off by one float
        wide = [torch.full((n, D + 12), 7.0, device=dev) for n in (B, B, N)]
        for w, k in zip(wide, ('query', 'item', 'extra_item')):
            w[:, col:col + D] = _t(case[k], dev)
        q, v, x = (w[:, col:col + D] for w in wide)
        before = _census()
        got = _run(case, dev, q=q, v=v, x=x)
        now = _census()
        assert _same(want, got)
        assert torch.equal(_bits(got.row_pos_logit), _bits(_terms(case, dev, q=q, v=v, x=x).row_pos_logit))
        if D == 64:                                    # the views themselves reached the kernel: guarded accesses for col 1
            vec = 1 if col == 4 else 0
            assert all(now[(w, vec)] == before[(w, vec)] + 1 and now[(w, 1 - vec)] == before[(w, 1 - vec)] for w in (0, 1, 2))
    xt = _t(case['extra_item'].T.copy(), dev).T        # column-major: made contiguous, same bits
    assert _same(want, _run(case, dev, x=xt))


# ---- 5. edge cases --------------------------------------------------------------------------------------------------------------------------
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
        assert (ref['n_greater'] >= 1).all() and np.abs(ref['pos']).max() <= 87.5 and max(s for r in ref['cands'] for _, s in r) == 100.0
        _exactly(_run(case, dev, in_batch), ref)
    full = K.ranks_of(case)
    case['extra_mask'] = np.ones(N, dtype=bool)        # without its greatest candidate a row's count drops by exactly one
    case['extra_mask'][c[7]] = False
    want = K.ranks_of(case)
    assert want['n_greater'][7] == full['n_greater'][7] - 1
    _exactly(_run(case, dev), want)


@pytest.mark.parametrize('B,N', [(1, 3), (R + 3, T + 7)])
def test_extras_that_are_all_hits_or_masked_are_nobodys_candidates(dev, B, N):
    case = K.exact_case(B, N, 33, 'log_q')
    case['extra_mask'] = np.zeros(N, dtype=bool)                          # all masked: the batch columns are left
    _exactly(_run(case, dev), K.ranks_of(case), 'masked')
    case['item_ids'] = np.full(B, 11, dtype=np.int64)                     # every other row is a hit; every second extra too, the others masked
    case['extra_item_ids'] = np.where(np.arange(N) % 2 == 0, 11, 12).astype(np.int64)
    case['extra_mask'] = np.arange(N) % 2 == 0
    for in_batch in (True, False):
        got = _run(case, dev, in_batch)
        assert not any(getattr(got, k).any().item() for k in COUNTS) and torch.isfinite(got.row_pos_logit).all() and got.n_rows.item() == B
        _exactly(got, K.ranks_of(case, in_batch_candidates=in_batch), 'hits')


def test_masked_rows_and_masked_extras_full_of_nan_and_inf_touch_no_bit(dev):
    B, N, D = 129, 97, 128
    case, _ = K.float_ref(B, N, D, 'all')
    off, xoff = ~case['mask'], ~case['extra_mask']
    fill = np.where(np.arange(D) % 3 == 0, np.nan, np.where(np.arange(D) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    for in_batch in (True, False):
        outs = []
        for bad in (False, True):
            c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
            for k, rows in (('query', off), ('item', off), ('extra_item', xoff)):
                c[k][rows] = fill if bad else 0.25
            c['log_q'][off] = np.nan if bad else 0.0
            c['extra_log_q'][xoff] = -np.inf if bad else 0.0
            outs.append(_run(c, dev, in_batch))
        assert off.sum() > T and xoff.sum() > T and _same(outs[0], outs[1])
        assert not torch.isnan(outs[1].row_pos_logit[torch.from_numpy(~off).to(dev)]).any()
        assert not any(getattr(outs[1], k)[torch.from_numpy(off).to(dev)].any().item() for k in COUNTS)


def test_a_nan_candidate_counts_as_greater_and_a_nan_positive_puts_every_candidate_above(dev):
    case, ref = K.exact_ref(197, 129, 64, 'mask')
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    k = np.flatnonzero(case['extra_mask'])[-1]
    c['extra_item'][k, 63] = np.nan                    # an extra every taking-part row sees
    i0 = np.flatnonzero(case['mask'])[5]
    c['item'][i0, 0] = np.nan                          # and a positive (a candidate of every other row)
    for in_batch in (True, False):
        want = K.ranks_of(c, in_batch_candidates=in_batch)
        base = ref if in_batch else K.exact_ref(197, 129, 64, 'mask', False)[1]
        assert want['n_greater'][i0] == want['n_candidates'][i0] > 0 and want['n_equal'][i0] == 0 and np.isnan(want['pos'][i0])
        assert (want['n_greater'][want['on']] > base['n_greater'][want['on']]).any()
        got = _run(c, dev, in_batch)
        _exactly(got, want)
        assert got.n_greater[i0].item() == got.n_candidates[i0].item() and torch.isnan(got.row_pos_logit[i0])


def test_a_row_that_is_its_own_only_candidate_has_three_zero_counts(dev):
    M = _mod()
    q, v = torch.full((1, 7), 0.5, device=dev), torch.full((1, 7), 2.0, device=dev)
    r = M.in_batch_ranks(q, v)
    assert [getattr(r, k).item() for k in COUNTS] == [0, 0, 0] and r.row_pos_logit.item() == 7.0 and r.n_rows.item() == 1
    m = M.in_batch_retrieval_metrics(q, v, k=(1, 3))
    assert m.recall.tolist() == [1.0, 1.0] and m.ndcg.tolist() == [1.0, 1.0] and m.mrr.item() == 1.0 and m.mean_rank.item() == 1.0
    r = M.in_batch_ranks(q, v, extra_item=torch.zeros((0, 7), device=dev), in_batch_candidates=False)      # an empty corpus
    assert [getattr(r, k).item() for k in COUNTS] == [0, 0, 0] and r.row_pos_logit.item() == 7.0


# ---- 6. launches and determinism -------------------------------------------------------------------------------------------------------------
def test_the_corpus_alone_leaves_the_item_segment_unwalked_and_is_the_masked_restatement(dev):
    B, N, D = 33, 32, 8
    for config in ('plain', 'all'):
        case, _ = K.exact_ref(B, N, D, config)
        before = _census()
        got = _np(_run(case, dev, False))
        now = _census()
        assert now[(3, 0)] == before[(3, 0)] + 1 and now[(3, 1)] == before[(3, 1)] and now[(1, 1)] == before[(1, 1)] + 1
        on = np.ones(B, dtype=bool) if case['mask'] is None else case['mask']
        for i in range(B):                                 # row i with every other batch row masked out of the candidate set
            m = np.zeros(B, dtype=bool)
            m[i] = on[i]
            one = _np(_run(case, dev, True, mask=_t(m, dev)))
            assert all(one[k][i] == got[k][i] for k in COUNTS)
            assert np.array_equal(one['row_pos_logit'][i:i + 1], got['row_pos_logit'][i:i + 1], equal_nan=True)
        assert _census()[(3, 1)] == now[(3, 1)] + B


def test_census_every_width_of_every_side_and_the_old_censuses_untouched(dev):
    lib = _lib.load()
    old = _old_census()
    before = _census()
    _run(K.float_ref(65, 1, 64, 'plain')[0], dev)          # 16-byte accesses throughout, the items walked
    _run(K.float_ref(2, 31, 3, 'plain')[0], dev, False)    # none, the items left to the tiles of the positives
    now = _census()
    assert all(now[key] == before[key] + 1 for key in now)
    case = K.float_ref(65, 1, 64, 'plain')[0]              # no extras: the extras' census does not move
    _mod().in_batch_ranks(_t(case['query'], dev), _t(case['item'], dev))
    last = _census()
    assert last[(2, 0)] == now[(2, 0)] and last[(2, 1)] == now[(2, 1)] and last[(0, 1)] == now[(0, 1)] + 1 and last[(3, 1)] == now[(3, 1)] + 1
    assert old == _old_census()                            # rank launches are in neither census of the loss
    assert lib.recnow_ibs_rank_launches(4, 0) < 0 and lib.recnow_ibs_rank_launches(0, 2) < 0 and lib.recnow_ibs_rank_launches(-1, 0) < 0


def test_repeated_runs_and_graph_replay_are_bit_for_bit(dev):
    M = _mod()
    case, _ = K.float_ref(197, 129, 64, 'all')
    assert _same(_run(case, dev), _run(case, dev)) and _same(_run(case, dev, False), _run(case, dev, False))
    q, v, x = (_t(case[k], dev) for k in ('query', 'item', 'extra_item'))
    kw = _kw(case, dev)

    def step():
        r = M.in_batch_ranks(q, v, extra_item=x, **kw)
        m = M.in_batch_retrieval_metrics(q, v, extra_item=x, k=(1, 10), **kw)
        return tuple(r) + tuple(m)
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
        assert all(torch.equal(a, b) for a, b in zip(outs[:3], eager[:3])) and torch.equal(_bits(outs[3]), _bits(eager[3]))
        assert all(torch.equal(a, b) for a, b in zip(outs[4:], eager[4:])) and outs[0].any() and 0.0 < outs[7].item() < 1.0


# ---- 7. metrics -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False], ids=['batch', 'corpus'])
@pytest.mark.parametrize('ties', ['expected', 'optimistic', 'pessimistic'])
@pytest.mark.parametrize('B,N,D,config', [(197, 129, 64, 'all'), (33, 32, 8, 'plain'), (129, 97, 128, 'mask')])
def test_the_metrics_are_the_oracles_on_the_gpus_own_counts(dev, B, N, D, config, ties, in_batch):
    M = _mod()
    case, ref = K.exact_ref(B, N, D, config, in_batch)     # exact inputs: ties in plenty
    k = (1, 5, B + N + 7)
    got = _np(_run(case, dev, in_batch))
    assert got['n_equal'].any() or not in_batch
    want = K.metrics_oracle(got['n_greater'], got['n_equal'], ref['on'], k, ties)
    m = M.in_batch_retrieval_metrics(_t(case['query'], dev), _t(case['item'], dev), extra_item=_t(case['extra_item'], dev),
                                     in_batch_candidates=in_batch, k=k, ties=ties, **_kw(case, dev))
    assert m.recall.shape == (3,) and m.recall.dtype == torch.float64 and m.ndcg.shape == (3,) and m.mrr.dim() == 0 and m.mean_rank.dim() == 0
    assert m.n_rows.item() == want['n'] == ref['n']
    for what in ('recall', 'ndcg', 'mrr', 'mean_rank'):
        err = np.abs(np.array(getattr(m, what).tolist()) - np.array(want[what])).max()
        assert err <= 1e-12, '%s: off by %.3g' % (what, err)
    assert abs(m.recall[2].item() - 1.0) <= 1e-12 and 0.0 < m.mrr.item() <= 1.0 and m.mean_rank.item() >= 1.0


# ---- 8. memory ------------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_holds_no_b_by_b_plus_n_matrix(dev):
    """in_batch_ranks at B 1024, N 3072, D 32: above the inputs, the outputs (three int64 counts, the positive's logit and n_rows), the
    per-row vectors as the kernel reads them (int64 ids where int32 came in, uint8 masks) and a 64 KB allowance; one (B, B + N) fp32 matrix
    would be 16 MB."""
    M = _mod()
    B, N, D = 1024, 3072, 32
    gen = torch.Generator(device='cpu').manual_seed(3)
    q, v = ((torch.randn(B, D, generator=gen) * 0.4).to(dev) for _ in range(2))
    x = (torch.randn(N, D, generator=gen) * 0.4).to(dev)
    ids = torch.randint(0, B // 4, (B,), generator=gen, dtype=torch.int32).to(dev)
    xids = torch.randint(0, B // 4, (N,), generator=gen, dtype=torch.int32).to(dev)
    lq, xlq = torch.rand(B, generator=gen).add_(0.05).log_().to(dev), torch.rand(N, generator=gen).add_(0.05).log_().to(dev)
    m, xm = (torch.rand(B, generator=gen) > 0.1).to(dev), (torch.rand(N, generator=gen) > 0.1).to(dev)

    def step():
        return M.in_batch_ranks(q, v, item_ids=ids, log_q=lq, temperature=0.7, mask=m, extra_item=x, extra_item_ids=xids, extra_log_q=xlq,
                                extra_mask=xm)
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = (3 * 8 + 4) * B + 8 + (8 + 2) * (B + N) + 65536          # outputs; int64 ids, bool and uint8 masks; the allowance
    assert r.n_greater.any() and r.n_rows.item() == m.sum().item()
    assert rise <= allowed < B * (B + N) * 4 // 16, 'in_batch_ranks rose %d bytes, allowed %d' % (rise, allowed)

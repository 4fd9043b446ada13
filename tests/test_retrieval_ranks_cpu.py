"""CPU: the fp64 oracle of the in-batch retrieval ranks and metrics (tests/_retrieval_ranks_oracle.py) pinned to a hand-worked example, to the
torch fp64 (B, B + N) composition and to the oracle of the loss; its defining properties; the tie policies; and everything of
rec_now_amd.rec_block.retrieval_metrics that needs no GPU: the prefix-table aggregation against the loops, argument errors, the CPU and
D > 128 refusals, the B = 0 path, the host-only entry points of the library, and the guard band of the GPU tests on their shapes."""
import math

import numpy as np
import pytest
import torch

import _in_batch_softmax_extra_oracle as X
import _retrieval_ranks_oracle as K
from rec_now_amd import _lib
from rec_now_amd.rec_block import retrieval_metrics as M

COUNTS = ('n_greater', 'n_equal', 'n_candidates')


def _tt(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or not t.is_floating_point() else t.to(dtype)


def _composition(c, dtype, **kw):
    return K.composition_counts(_tt(c['query'], dtype), _tt(c['item'], dtype), _tt(c['extra_item'], dtype), _tt(c['item_ids']),
                                _tt(c['log_q'], dtype), c['temperature'], _tt(c['mask']), _tt(c['extra_item_ids']),
                                _tt(c['extra_log_q'], dtype), _tt(c['extra_mask']), **kw)


def _hand():
    """B = 3, N = 2, D = 2, tau = 1.  Logits (batch | extras), positives on the diagonal:
         row 0:  [1     0    0.25 | 1  2]     one tie (extra 0), one above (extra 1)
         row 1:  [0     2    0.5  | 1  0]     nothing above
         row 2:  [1     2    0.75 | 2  2]     everything above"""
    return dict(query=np.array([[1., 0.], [0., 1.], [1., 1.]]), item=np.array([[1., 0.], [0., 2.], [0.25, 0.5]]),
                extra_item=np.array([[1., 1.], [2., 0.]]), item_ids=None, log_q=None, temperature=1.0, mask=None, extra_item_ids=None,
                extra_log_q=None, extra_mask=None)


def test_a_hand_worked_example():
    c = _hand()
    r = K.ranks_of(c)
    assert r['n_greater'].tolist() == [1, 0, 4] and r['n_equal'].tolist() == [1, 0, 0] and r['n_candidates'].tolist() == [4, 4, 4]
    assert r['pos'].tolist() == [1.0, 2.0, 0.75] and r['n'] == 3
    # the corpus alone: the batch columns are nobody's candidates
    f = K.ranks_of(c, in_batch_candidates=False)
    assert f['n_greater'].tolist() == [1, 0, 2] and f['n_equal'].tolist() == [1, 0, 0] and f['n_candidates'].tolist() == [2, 2, 2]
    assert f['pos'].tolist() == [1.0, 2.0, 0.75]
    # extra 0 carries row 0's id: row 0 loses its tie, the others keep the extra
    i = K.ranks_of(c, item_ids=[5, 6, 7], extra_item_ids=[5, 9])
    assert i['n_greater'].tolist() == [1, 0, 4] and i['n_equal'].tolist() == [0, 0, 0] and i['n_candidates'].tolist() == [3, 4, 4]
    # row 1 does not take part: zeros and NaN for it, and one candidate fewer for the others
    m = K.ranks_of(c, mask=[1, 0, 1])
    assert m['n_greater'].tolist() == [1, 0, 3] and m['n_candidates'].tolist() == [3, 0, 3] and math.isnan(m['pos'][1]) and m['n'] == 2
    # a logQ correction of 1.5 on extra 0 alone takes it below both positives it tied or beat
    lq = K.ranks_of(c, log_q=np.zeros(3), extra_log_q=np.array([1.5, 0.0]))
    assert lq['n_greater'].tolist() == [1, 0, 3] and lq['n_equal'].tolist() == [0, 0, 0]
    # the metrics: ranks {2, 3}, {1}, {5}
    on = [True] * 3
    e = K.metrics_oracle(r['n_greater'], r['n_equal'], on, (1, 2), 'expected')
    assert np.allclose(e['recall'], [1 / 3, 0.5], rtol=1e-15) and abs(e['mrr'] - ((1 / 2 + 1 / 3) / 2 + 1 + 1 / 5) / 3) <= 1e-15
    assert np.allclose(e['ndcg'], [1 / 3, (0.5 / math.log2(3) + 1) / 3], rtol=1e-15) and abs(e['mean_rank'] - (2.5 + 1 + 5) / 3) <= 1e-15
    o = K.metrics_oracle(r['n_greater'], r['n_equal'], on, (1, 2), 'optimistic')
    assert np.allclose(o['recall'], [1 / 3, 2 / 3], rtol=1e-15) and abs(o['mrr'] - (1 / 2 + 1 + 1 / 5) / 3) <= 1e-15
    p = K.metrics_oracle(r['n_greater'], r['n_equal'], on, (1, 2), 'pessimistic')
    assert np.allclose(p['recall'], [1 / 3, 1 / 3], rtol=1e-15) and abs(p['mean_rank'] - (3 + 1 + 5) / 3) <= 1e-15


@pytest.mark.parametrize('in_batch', [True, False])
@pytest.mark.parametrize('config', X.CONFIGS)
@pytest.mark.parametrize('B,N,D', [(1, 1, 3), (7, 4, 5), (41, 37, 16)])
def test_the_oracle_counts_are_those_of_the_torch_fp64_composition(B, N, D, config, in_batch):
    for c in (X.make_extra_case(B, N, D, config, 16, 8), K.exact_case(B, N, D, config)):       # the second: ties
        r = K.ranks_of(c, in_batch_candidates=in_batch)
        g, e, n, pos = _composition(c, torch.float64, in_batch_candidates=in_batch)
        assert all(np.array_equal(r[k], t.numpy()) for k, t in zip(COUNTS, (g, e, n)))
        assert np.array_equal(r['pos'], pos.numpy(), equal_nan=True) or np.nanmax(np.abs(r['pos'] - pos.numpy())) <= 1e-13
    if B == 41 and config == 'plain' and in_batch:         # integer logits of a few dozen values: the exact case has ties
        assert r['n_equal'].sum() > 0


@pytest.mark.parametrize('config', X.CONFIGS)
def test_invariants(config):
    B, N, D = 29, 21, 5
    c = X.make_extra_case(B, N, D, config, 8, 8)
    r = K.ranks_of(c)
    assert (r['n_greater'] + r['n_equal'] <= r['n_candidates']).all() and r['n_candidates'].any()
    p = X.oracle_of(c)['p']                                # the candidates of the loss: its non-zero p entries, off the diagonal
    assert np.array_equal(r['n_candidates'], (p != 0).sum(axis=1) - (np.diagonal(p[:, :B]) != 0))
    assert np.array_equal(np.isnan(r['pos']), ~r['on']) and not r['n_candidates'][~r['on']].any()
    perm = np.random.default_rng(3).permutation(B)         # a permutation of the rows permutes the outputs
    rows = {k: (None if c[k] is None else c[k][perm]) for k in ('query', 'item', 'item_ids', 'log_q', 'mask')}
    a = K.ranks_of(c, **rows)
    assert all(np.array_equal(a[k], r[k][perm]) for k in COUNTS) and np.allclose(a['pos'], r['pos'][perm], rtol=0, atol=1e-13, equal_nan=True)
    xperm = np.random.default_rng(4).permutation(N)        # a permutation of the extras changes nothing
    b = K.ranks_of(c, **{k: (None if c[k] is None else c[k][xperm]) for k in ('extra_item',) + X.EXTRA_KEYS})
    assert all(np.array_equal(b[k], r[k]) for k in COUNTS)
    if c['log_q'] is not None:                             # a constant on both log_q changes nothing (3.25: exact in the sums at hand)
        d = K.ranks_of(K.exact_case(B, N, D, config))
        e = K.exact_case(B, N, D, config)
        e.update(log_q=e['log_q'] + 3.25, extra_log_q=e['extra_log_q'] + 3.25)
        assert all(np.array_equal(K.ranks_of(e)[k], d[k]) for k in COUNTS)
    for case in (c, K.exact_case(B, N, D, config)):        # the corpus alone is the call with every other batch row masked out
        f, want = K.ranks_of(case, in_batch_candidates=False), K.without_batch_candidates_as_a_mask(case)
        assert all(np.array_equal(f[k], want[k]) for k in COUNTS) and np.array_equal(f['pos'], want['pos'], equal_nan=True)


def test_a_nan_counts_as_greater():
    c = _hand()
    c['extra_item'] = np.array([[1., 1.], [np.nan, 0.]])
    r = K.ranks_of(c)
    assert r['n_greater'].tolist() == [1, 1, 4] and r['n_equal'].tolist() == [1, 0, 0]
    c = _hand()
    c['item'][1, 1] = np.nan                               # row 1's positive is NaN; rows 0 and 2 see NaN * 0 and 1 * NaN in column 1
    r = K.ranks_of(c)
    assert r['n_greater'].tolist() == [2, 4, 4] and r['n_equal'].tolist() == [1, 0, 0]


# ---- tie policies ----------------------------------------------------------------------------------------------------------------------------
def _counts(seed, B=57, top=40, ties=True):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, top, B)
    e = rng.integers(0, 6, B) * (rng.random(B) < 0.5) if ties else np.zeros(B, dtype=np.int64)
    on = rng.random(B) < 0.8
    g[~on], e[~on] = 0, 0
    return g.astype(np.int64), e.astype(np.int64), on


def _table_form(g, e, on, n_ranks, k, ties):
    m = M.metrics_from_counts(torch.from_numpy(g), torch.from_numpy(e), torch.from_numpy(on), torch.tensor(int(on.sum())), n_ranks, k, ties)
    assert m.recall.dtype == torch.float64 and m.recall.shape == (len(k),) and m.ndcg.shape == (len(k),) and m.mrr.dim() == 0
    return dict(recall=m.recall.tolist(), ndcg=m.ndcg.tolist(), mrr=m.mrr.item(), mean_rank=m.mean_rank.item())


@pytest.mark.parametrize('ties', M.TIES)
def test_the_prefix_table_form_is_the_loop_form(ties):
    k = (1, 5, 10, 52, 1000)
    for seed in range(3):
        g, e, on = _counts(seed)
        want, got = K.metrics_oracle(g, e, on, k, ties), _table_form(g, e, on, 57 + 40 + 1, k, ties)
        for what in ('recall', 'ndcg', 'mrr', 'mean_rank'):
            assert np.abs(np.array(got[what]) - np.array(want[what])).max() <= 1e-12, what
    none = np.zeros(5, dtype=bool)                         # no row takes part: every mean is 0
    got = _table_form(np.zeros(5, np.int64), np.zeros(5, np.int64), none, 9, k, ties)
    assert got['mrr'] == 0.0 and got['mean_rank'] == 0.0 and not any(got['recall']) and not any(got['ndcg'])


def test_the_three_policies_agree_without_ties_and_are_ordered_with_them():
    k = (1, 3, 20)
    g, e, on = _counts(5, ties=False)
    o, x, p = (K.metrics_oracle(g, e, on, k, t) for t in ('optimistic', 'expected', 'pessimistic'))
    assert o == x == p
    g, e, on = _counts(6)
    o, x, p = (K.metrics_oracle(g, e, on, k, t) for t in ('optimistic', 'expected', 'pessimistic'))
    for what in ('recall', 'ndcg', 'mrr'):
        a, b, c = (np.atleast_1d(np.array(t[what])) for t in (o, x, p))
        assert (a >= b).all() and (b >= c).all() and (a > c).any(), what
    assert o['mean_rank'] < x['mean_rank'] < p['mean_rank']


def test_all_equal_logits_give_recall_k_over_c_plus_one_under_expected():
    """A collapsed tower: every logit equal, c candidates beside the positive, all of them ties."""
    B, N = 6, 9
    c = dict(query=np.ones((B, 4)), item=np.ones((B, 4)), extra_item=np.ones((N, 4)), item_ids=None, log_q=None, temperature=1.0, mask=None,
             extra_item_ids=None, extra_log_q=None, extra_mask=None)
    r = K.ranks_of(c)
    cc = B - 1 + N
    assert (r['n_equal'] == cc).all() and not r['n_greater'].any()
    on = np.ones(B, dtype=bool)
    for kk in (1, 3, cc + 1):
        want = kk / (cc + 1)
        assert abs(K.metrics_oracle(r['n_greater'], r['n_equal'], on, (kk,), 'expected')['recall'][0] - want) <= 1e-15
        assert abs(_table_form(r['n_greater'], r['n_equal'], on, B + N + 1, (kk,), 'expected')['recall'][0] - want) <= 1e-12
    assert K.metrics_oracle(r['n_greater'], r['n_equal'], on, (1,), 'optimistic')['recall'][0] == 1.0
    assert K.metrics_oracle(r['n_greater'], r['n_equal'], on, (cc,), 'pessimistic')['recall'][0] == 0.0


# ---- the module without a GPU ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    i4, i5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int32)
    for f in (M.in_batch_ranks, M.in_batch_retrieval_metrics):
        for bad in (lambda: f(q, torch.zeros(4, 2)), lambda: f(q, v, temperature=0.0), lambda: f(q, v, mask=torch.ones(3)),
                    lambda: f(q, v, item_ids=torch.zeros(4)),                                                            # those of the loss
                    lambda: f(q, v, extra_item=torch.zeros(5, 2)), lambda: f(q, v, item_ids=i4, extra_item=x),
                    lambda: f(q, v, extra_item=x, extra_item_ids=i5), lambda: f(q, v, log_q=torch.zeros(4), extra_item=x),
                    lambda: f(q, v, extra_mask=torch.ones(5)),                                                           # those of the extras
                    lambda: f(q, v, in_batch_candidates=False),                                                          # a corpus is required
                    lambda: f(q, v, item_ids=i4, in_batch_candidates=False)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(NotImplementedError):
            f(torch.zeros(4, 129), torch.zeros(4, 129))
        with pytest.raises(TypeError):                     # keyword-only
            f(q, v, None, None, 1.0, None, True, x)
    f = M.in_batch_retrieval_metrics
    for bad in (lambda: f(q, v, k=()), lambda: f(q, v, k=(1, 0)), lambda: f(q, v, k=(-3,)), lambda: f(q, v, k=(2.0,)), lambda: f(q, v, k=(True,)),
                lambda: f(q, v, k='10'), lambda: f(q, v, k=None), lambda: f(q, v, ties='mean'), lambda: f(q, v, ties=None)):
        with pytest.raises(ValueError):                    # before the CPU refusal
            bad()


def test_cpu_tensors_are_refused_after_the_argument_checks():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    kw = dict(item_ids=torch.zeros(4, 1, dtype=torch.int32), log_q=torch.zeros(4, 1), extra_item=x,
              extra_item_ids=torch.zeros(5, 1, dtype=torch.int32), extra_log_q=torch.zeros(5, 1), extra_mask=torch.ones(5))
    for f in (M.in_batch_ranks, M.in_batch_retrieval_metrics):
        with pytest.raises(RuntimeError, match='only on the GPU'):
            f(q, v, **kw)
        with pytest.raises(RuntimeError, match='only on the GPU'):
            f(q, v, extra_item=x, in_batch_candidates=False)
        with pytest.raises(ValueError):
            f(q, v, **dict(kw, extra_log_q=None))


def test_an_empty_batch_is_empty_counts_and_zero_metrics_without_a_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', boom)
    monkeypatch.setattr(_lib, 'load', boom)
    q, v, x = torch.zeros(0, 8), torch.zeros(0, 8), torch.full((5, 8), float('nan'))
    for in_batch in (True, False):
        r = M.in_batch_ranks(q, v, extra_item=x, in_batch_candidates=in_batch)
        assert all(t.shape == (0,) and t.dtype == torch.int64 for t in r[:3]) and r.row_pos_logit.shape == (0,)
        assert r.row_pos_logit.dtype == torch.float32 and r.n_rows.item() == 0 and r.n_rows.dim() == 0
        m = M.in_batch_retrieval_metrics(q, v, extra_item=x, in_batch_candidates=in_batch, k=(1, 7))
        assert m.recall.tolist() == [0.0, 0.0] and m.ndcg.tolist() == [0.0, 0.0] and m.recall.dtype == torch.float64
        assert m.mrr.item() == 0.0 and m.mean_rank.item() == 0.0 and m.mrr.dim() == 0 and m.n_rows.item() == 0


def test_abi_and_host_only_entry_points():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 32 and lib.recnow_abi_version() >= 32
    assert all(lib.recnow_ibs_rank_launches(w, vec) >= 0 for w in range(4) for vec in (0, 1))
    assert all(lib.recnow_ibs_rank_launches(w, vec) < 0 for w, vec in ((-1, 0), (4, 0), (0, -1), (0, 2), (3, 2)))


def test_the_rank_call_checks_its_arguments():
    """The checks of recnow_ibs_extra_fwd, N = 0 allowed, and no launch without its outputs (all pointers are host memory or NULL here:
    nothing could run)."""
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(1))

    def rank(B=4, D=1, x=p, ldx=1, ids=None, xids=None, N=1, inv_tau=1.0, batch=1, out=None, ldq=1):
        return lib.recnow_ibs_rank(p, ldq, p, 1, ids, None, None, B, D, x, ldx, xids, None, None, N, inv_tau, 1, batch, out, out, out, None, None)
    EINVAL, EUNSUPPORTED = -1, -3
    census = [lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)]
    assert rank(N=-1) == EINVAL and rank(ldx=0) == EINVAL and rank(x=None) == EINVAL and rank(N=(1 << 30) + 1) == EUNSUPPORTED
    assert rank(ids=p) == EINVAL and rank(xids=p) == EINVAL                 # ids come in pairs
    assert rank(B=-1) == EINVAL and rank(D=129) == EUNSUPPORTED and rank(ldq=0) == EINVAL and rank(B=(1 << 30) + 1) == EUNSUPPORTED
    assert rank(B=0) == 0 and rank(B=0, N=0, x=None) == 0 and rank(B=0, batch=0) == 0          # no row: nothing to do
    assert rank() == EINVAL and rank(N=0, x=None) == EINVAL and rank(batch=0) == EINVAL     # good arguments, no outputs: refused
    assert rank(out=p, inv_tau=0.0) == EINVAL                              # (row_pos is still NULL)
    assert census == [lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)]        # and nothing was launched


# ---- the guard band of the float regime, on the GPU shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False])
@pytest.mark.parametrize('config', X.CONFIGS)
def test_the_fp32_composition_lies_inside_the_guard_band(config, in_batch):
    for B, N, D in X.SHAPES:
        c, r = K.float_ref(B, N, D, config, in_batch)
        g, e, n, pos = (t.numpy() for t in _composition(c, torch.float32, in_batch_candidates=in_batch))
        assert np.array_equal(n, r['n_candidates']), (B, N, D)
        assert (r['g_lo'] <= g).all() and (g + e <= r['g_hi']).all(), (B, N, D)
        on = r['on']
        assert np.isnan(pos[~on]).all() and (np.abs(pos[on] - r['pos'][on]) <= 1e-6 * np.maximum(1.0, np.abs(r['pos'][on]))).all()


def test_the_guard_band_is_narrow():
    """At most 2 % of a case's taking-part rows are ambiguous (G_lo != G_hi), and some case has none: the band decides nearly every row."""
    worst, total, rows, clean = 0.0, 0, 0, 0
    for in_batch in (True, False):
        for B, N, D in X.SHAPES:
            for config in X.CONFIGS:
                r = K.float_ref(B, N, D, config, in_batch)[1]
                if r['n'] == 0:
                    continue
                amb = int((r['g_lo'] != r['g_hi']).sum())
                assert (r['g_lo'] <= r['n_greater']).all() and (r['n_greater'] + r['n_equal'] <= r['g_hi']).all()
                assert amb <= 0.02 * r['n'], (B, N, D, config, amb, r['n'])
                worst, total, rows, clean = max(worst, amb / r['n']), total + amb, rows + r['n'], clean + (amb == 0)
    print('ambiguous rows: %d of %d; worst case %.2f %%; %d cases with none' % (total, rows, 100 * worst, clean))
    assert clean >= 1

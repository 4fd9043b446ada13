"""CPU: the fp64 oracle of the in-batch top-K candidates (tests/_retrieval_topk_oracle.py) pinned to a hand-worked example and to the torch
fp64 (B, B + N) composition + topk; its defining properties (prefix, corpus mode as a mask, permutation of the extras); and everything of
rec_now_amd.rec_block.retrieval_topk that needs no GPU: argument errors, the ceiling, the CPU and D > 128 refusals, the B = 0 path, the
host-only entry points of the library, and the float-regime contract of the GPU tests held by the fp32 torch composition on their shapes."""
import numpy as np
import pytest
import torch

import _in_batch_softmax_extra_oracle as X
import _retrieval_ranks_oracle as K
import _retrieval_topk_oracle as O
from rec_now_amd import _lib
from rec_now_amd.rec_block import retrieval_topk as M

INF = float('inf')


def _hand():
    """B = 3, N = 2, D = 2, tau = 1.  Logits (batch | extras), positives on the diagonal:
         row 0:  [1     0    0.25 | 1  2]
         row 1:  [0     2    0.5  | 1  0]     columns 0 and 4 tie at 0
         row 2:  [1     2    0.75 | 2  2]     columns 1, 3 and 4 tie at 2"""
    return dict(query=np.array([[1., 0.], [0., 1.], [1., 1.]]), item=np.array([[1., 0.], [0., 2.], [0.25, 0.5]]),
                extra_item=np.array([[1., 1.], [2., 0.]]), item_ids=None, log_q=None, temperature=1.0, mask=None, extra_item_ids=None,
                extra_log_q=None, extra_mask=None)


def test_the_total_order():
    nan = float('nan')
    assert O.before(nan, 9, INF, 0) and not O.before(INF, 0, nan, 9)            # NaN is greatest
    assert O.before(nan, 1, nan, 2) and not O.before(nan, 2, nan, 1)            # two NaNs: by index
    assert O.before(2.0, 9, 1.0, 0) and not O.before(1.0, 0, 2.0, 9)
    assert O.before(-0.0, 1, 0.0, 2) and O.before(0.0, 1, -0.0, 2) and not O.before(0.0, 2, -0.0, 1)      # the zeros tie
    assert O.before(-INF, 0, -INF, 1) and O.before(1.0, 5, -INF, 0)
    got = O.sort_total([(0, 1.0), (1, nan), (2, 1.0), (3, -INF), (4, 7.0), (5, nan), (6, -0.0), (7, 0.0)])
    assert [j for j, _ in got] == [1, 5, 4, 0, 2, 6, 7, 3]


def test_a_hand_worked_example():
    c = _hand()
    s, i, n = O.topk_oracle(O.ranks_of(c), 3)
    assert i.tolist() == [[4, 3, 2], [3, 2, 0], [1, 3, 4]] and s.tolist() == [[2, 1, 0.25], [1, 0.5, 0], [2, 2, 2]] and n.tolist() == [4, 4, 4]
    s, i, n = O.topk_oracle(O.ranks_of(c), 5)              # fewer than K candidates: the fill
    assert i.tolist() == [[4, 3, 2, 1, -1], [3, 2, 0, 4, -1], [1, 3, 4, 0, -1]]
    assert s.tolist() == [[2, 1, 0.25, 0, -INF], [1, 0.5, 0, 0, -INF], [2, 2, 2, 1, -INF]]
    # the corpus alone: indices still address cat(item, extra_item)
    s, i, n = O.topk_oracle(O.ranks_of(c, in_batch_candidates=False), 3)
    assert i.tolist() == [[4, 3, -1], [3, 4, -1], [3, 4, -1]] and s.tolist() == [[2, 1, -INF], [1, 0, -INF], [2, 2, -INF]] and n.tolist() == [2, 2, 2]
    # extra 1 carries row 2's id: removed for row 2 alone; row 1 does not take part: all fill, and nobody's candidate
    s, i, n = O.topk_oracle(O.ranks_of(c, item_ids=[5, 6, 7], extra_item_ids=[9, 7], mask=[1, 0, 1]), 2)
    assert i.tolist() == [[4, 3], [-1, -1], [3, 0]] and s.tolist() == [[2, 1], [-INF, -INF], [2, 1]] and n.tolist() == [3, 0, 2]
    # a candidate at -inf is a candidate: it carries its index and stands before the fill
    s, i, n = O.topk_oracle(O.ranks_of(c, log_q=np.zeros(3), extra_log_q=np.array([INF, 0.0])), 5)
    assert i[0].tolist() == [4, 2, 1, 3, -1] and s[0].tolist() == [2, 0.25, 0, -INF, -INF]


@pytest.mark.parametrize('in_batch', [True, False])
@pytest.mark.parametrize('config', X.CONFIGS)
@pytest.mark.parametrize('B,N,D', [(1, 1, 3), (7, 4, 5), (41, 37, 16)])
def test_the_oracle_is_the_torch_fp64_composition_wherever_a_row_has_no_ties(B, N, D, config, in_batch):
    rows = 0
    for c in (X.make_extra_case(B, N, D, config, 16, 8), K.exact_case(B, N, D, config)):
        ref = O.ranks_of(c, in_batch_candidates=in_batch)
        for k in (1, 4, 128):
            s, i, n = O.topk_oracle(ref, k)
            ts, ti, tn, _ = O.composition_of(c, k, torch.float64, in_batch)
            assert np.array_equal(n, tn.numpy())
            for r in range(B):
                vals = [v for _, v in ref['cands'][r]]
                if len(set(vals)) == len(vals):            # no ties: topk has no choice
                    rows += 1
                    assert np.array_equal(i[r], ti[r].numpy()), (k, r)
                    assert np.allclose(s[r], ts[r].numpy(), rtol=0, atol=1e-13), (k, r)
                else:                                      # ties: the scores agree, the indices are the oracle's to order
                    assert np.allclose(s[r], ts[r].numpy(), rtol=0, atol=1e-13), (k, r)
    assert rows > 0


@pytest.mark.parametrize('in_batch', [True, False])
@pytest.mark.parametrize('config', X.CONFIGS)
def test_the_prefix_property_and_the_candidate_count(config, in_batch):
    for c in (X.make_extra_case(29, 150, 5, config, 8, 8), K.exact_case(29, 150, 5, config)):
        ref = O.ranks_of(c, in_batch_candidates=in_batch)
        s128, i128, n128 = O.topk_oracle(ref, 128)
        s5, i5, n5 = O.topk_oracle(ref, 5)
        assert np.array_equal(s5, s128[:, :5]) and np.array_equal(i5, i128[:, :5]) and np.array_equal(n5, n128)
        assert np.array_equal(n128, ref['n_candidates']) and ((i128 >= 0).sum(1) == np.minimum(128, n128)).all()
        assert not (i128[ref['on']] == np.arange(29)[ref['on'], None]).any()              # the positive is never in the list
        # agreement with the counts: the entries above the positive are the first min(K, n_greater)
        above = np.array([sum(1 for v in s5[r][i5[r] >= 0] if not (v <= ref['pos'][r])) for r in range(29)])
        assert np.array_equal(above[ref['on']], np.minimum(5, ref['n_greater'])[ref['on']])


@pytest.mark.parametrize('config', X.CONFIGS)
def test_the_corpus_alone_is_the_call_with_every_other_batch_row_masked_out(config):
    B, N, D = 13, 21, 5
    for c in (X.make_extra_case(B, N, D, config, 8, 8), K.exact_case(B, N, D, config)):
        s, i, n = O.topk_oracle(O.ranks_of(c, in_batch_candidates=False), 7)
        on = np.ones(B, dtype=bool) if c['mask'] is None else np.asarray(c['mask']).reshape(-1) != 0
        for r in range(B):
            m = np.zeros(B, dtype=bool)
            m[r] = on[r]
            s1, i1, n1 = O.topk_oracle(O.ranks_of(c, mask=m), 7)
            assert np.array_equal(s1[r], s[r]) and np.array_equal(i1[r], i[r]) and n1[r] == n[r]


@pytest.mark.parametrize('in_batch', [True, False])
def test_a_permutation_of_the_extras_permutes_the_indices_by_its_inverse(in_batch):
    B, N, D = 11, 23, 6
    c = X.make_extra_case(B, N, D, 'all', 8, 8)
    ref = O.ranks_of(c, in_batch_candidates=in_batch)
    assert all(len({v for _, v in row}) == len(row) for row in ref['cands'])      # no ties
    s, i, n = O.topk_oracle(ref, 9)
    perm = np.random.default_rng(4).permutation(N)             # new extra k is old extra perm[k]
    d = dict(c, **{k: c[k][perm] for k in ('extra_item',) + X.EXTRA_KEYS})
    s2, i2, n2 = O.topk_oracle(O.ranks_of(d, in_batch_candidates=in_batch), 9)
    back = np.where(i2 >= B, B + perm[np.clip(i2 - B, 0, N - 1)], i2)
    assert np.array_equal(s2, s) and np.array_equal(back, i) and np.array_equal(n2, n) and (i >= B).any()


# ---- the module without a GPU ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_ceiling():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    i4, i5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int32)
    f = M.in_batch_top_k
    for bad in (lambda: f(q, torch.zeros(4, 2), k=1), lambda: f(q, v, temperature=0.0, k=1), lambda: f(q, v, mask=torch.ones(3), k=1),
                lambda: f(q, v, item_ids=torch.zeros(4), k=1),                                                            # those of the loss
                lambda: f(q, v, extra_item=torch.zeros(5, 2), k=1), lambda: f(q, v, item_ids=i4, extra_item=x, k=1),
                lambda: f(q, v, extra_item=x, extra_item_ids=i5, k=1), lambda: f(q, v, log_q=torch.zeros(4), extra_item=x, k=1),
                lambda: f(q, v, extra_mask=torch.ones(5), k=1),                                                           # those of the extras
                lambda: f(q, v, in_batch_candidates=False, k=1), lambda: f(q, v, item_ids=i4, in_batch_candidates=False, k=1),
                lambda: f(q, v, k=0), lambda: f(q, v, k=-2), lambda: f(q, v, k=True), lambda: f(q, v, k=2.0), lambda: f(q, v, k='3'),
                lambda: f(q, v, k=None), lambda: f(q, v, k=(1, 2))):
        with pytest.raises(ValueError):                        # before the CPU refusal
            bad()
    with pytest.raises(TypeError):                             # k is required, and keyword-only
        f(q, v)
    with pytest.raises(TypeError):
        f(q, v, None, None, 1.0, None, True, 3)
    with pytest.raises(NotImplementedError):
        f(torch.zeros(4, 129), torch.zeros(4, 129), k=1)
    assert M.MAX_K == _lib.load().recnow_ibs_topk_max_k() == 128
    with pytest.raises(NotImplementedError, match='at most 128'):
        f(q, v, k=129)
    with pytest.raises(NotImplementedError):
        f(torch.zeros(0, 3), torch.zeros(0, 3), k=129)


def test_cpu_tensors_are_refused_after_the_argument_checks():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    kw = dict(item_ids=torch.zeros(4, 1, dtype=torch.int32), log_q=torch.zeros(4, 1), extra_item=x,
              extra_item_ids=torch.zeros(5, 1, dtype=torch.int32), extra_log_q=torch.zeros(5, 1), extra_mask=torch.ones(5))
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_top_k(q, v, k=2, **kw)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_top_k(q, v, k=128, extra_item=x, in_batch_candidates=False)
    with pytest.raises(ValueError):
        M.in_batch_top_k(q, v, k=2, **dict(kw, extra_log_q=None))


def test_an_empty_batch_is_empty_outputs_without_a_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', boom)
    monkeypatch.setattr(_lib, 'load', boom)
    q, v, x = torch.zeros(0, 8), torch.zeros(0, 8), torch.full((5, 8), float('nan'))
    for in_batch in (True, False):
        for k in (1, 7, 128):
            r = M.in_batch_top_k(q, v, k=k, extra_item=x, in_batch_candidates=in_batch)
            assert r.scores.shape == (0, k) and r.scores.dtype == torch.float32 and r.indices.shape == (0, k) and r.indices.dtype == torch.int64
            assert r.n_candidates.shape == (0,) and r.n_candidates.dtype == torch.int64


def test_abi_and_host_only_entry_points():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 33 and lib.recnow_abi_version() >= 33
    assert lib.recnow_ibs_topk_max_k() == 128
    assert all(lib.recnow_ibs_topk_launches(w, vec) >= 0 for w in range(4) for vec in (0, 1))
    assert all(lib.recnow_ibs_topk_launches(w, vec) < 0 for w, vec in ((-1, 0), (4, 0), (0, -1), (0, 2), (3, 2)))


def test_the_top_k_call_checks_its_arguments():
    """The checks of recnow_ibs_rank, then K, the outputs and their leading dimensions (all pointers are host memory or NULL here: nothing
    could run)."""
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(1))

    def topk(B=4, D=1, x=p, ldx=1, ids=None, xids=None, N=1, inv_tau=1.0, batch=1, K=1, s=None, lds=1, i=None, ldi=1, n=None, ldq=1):
        return lib.recnow_ibs_topk(p, ldq, p, 1, ids, None, None, B, D, x, ldx, xids, None, None, N, inv_tau, 1, batch, K, s, lds, i, ldi, n, None)
    EINVAL, EUNSUPPORTED = -1, -3
    census = [lib.recnow_ibs_topk_launches(w, vec) for w in range(4) for vec in (0, 1)]
    old = [lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)]
    assert topk(N=-1) == EINVAL and topk(ldx=0) == EINVAL and topk(x=None) == EINVAL and topk(N=(1 << 30) + 1) == EUNSUPPORTED
    assert topk(ids=p) == EINVAL and topk(xids=p) == EINVAL                 # ids come in pairs
    assert topk(B=-1) == EINVAL and topk(D=129) == EUNSUPPORTED and topk(ldq=0) == EINVAL and topk(B=(1 << 30) + 1) == EUNSUPPORTED
    assert topk(B=0) == 0 and topk(B=0, N=0, x=None) == 0 and topk(B=0, batch=0) == 0 and topk(B=0, K=128) == 0      # no row: nothing to do
    assert topk(K=0) == EINVAL and topk(K=-1) == EINVAL and topk(B=0, K=0) == EINVAL
    assert topk(K=129, s=p, i=p, n=p, lds=129, ldi=129) == EUNSUPPORTED and topk(B=0, K=129) == EUNSUPPORTED
    assert topk() == EINVAL and topk(N=0, x=None) == EINVAL and topk(batch=0) == EINVAL     # good arguments, no outputs: refused
    assert topk(s=p, i=p) == EINVAL and topk(s=p, n=p) == EINVAL and topk(i=p, n=p) == EINVAL
    assert topk(K=2, s=p, i=p, n=p, lds=1, ldi=2) == EINVAL and topk(K=2, s=p, i=p, n=p, lds=2, ldi=1) == EINVAL
    assert topk(s=p, i=p, n=p, inv_tau=0.0) == EINVAL
    assert census == [lib.recnow_ibs_topk_launches(w, vec) for w in range(4) for vec in (0, 1)]        # and nothing was launched
    assert old == [lib.recnow_ibs_rank_launches(w, vec) for w in range(4) for vec in (0, 1)]


# ---- the float regime, on the GPU shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_batch', [True, False])
@pytest.mark.parametrize('config', X.CONFIGS)
def test_the_fp32_composition_holds_the_float_regime_contract(config, in_batch):
    """The contract the GPU test holds the kernel to, held here by the fp32 torch composition: every GPU shape, K 1, 5, 33, 128.  The
    kept set equals fp64's in every row of these inputs."""
    worst, rows = (0.0, 0.0), 0
    for B, N, D in O.SHAPES:
        c, ref = O.float_ref(B, N, D, config, in_batch)
        for k in O.KS:
            s, i, n, _ = (t.numpy() for t in O.composition_of(c, k, torch.float32, in_batch))
            w = O.check_float_regime(s, i, n, ref, k)
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
            es, ei, _ = O.topk_oracle(ref, k)
            assert all(set(i[r]) == set(ei[r]) for r in range(B)), (B, N, D, k)
        rows += ref['n']
    print('%d taking-part rows; worst score error %.2f of the bound; worst excluded candidate %.2f of its bound' % (rows, worst[0], worst[1]))
    assert worst[1] <= 0.0                                    # no excluded candidate lies above the last kept one at all

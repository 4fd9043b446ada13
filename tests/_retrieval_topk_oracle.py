"""fp64 oracle of the in-batch top-K candidates (rec_now_amd/rec_block/retrieval_topk.py): the candidate lists of the rank oracle
(tests/_retrieval_ranks_oracle.py: per row, per candidate, the batch columns then the extras, never a matrix expression), put in the total
order by a plain insertion loop.  Plus the (B, B + N) torch composition a user writes without the fused kernel, and the checks of the
float regime that the CPU and GPU test files share."""
import functools
import math

import numpy as np

from _retrieval_ranks_oracle import CONFIGS, EXACT_SHAPES, R, SHAPES, T, exact_ref, float_ref, ranks_of, ranks_oracle, shape_case  # noqa: F401

KS = (1, 5, 33, 128)
LOGIT = 1e-6                                   # the project's per-logit bound
GUARD = 2e-6                                   # ... once for each of the two logits compared


def before(sa, ia, sb, ib):
    """Candidate a (score, index) stands before candidate b: the total order of the definition."""
    a_nan, b_nan = math.isnan(sa), math.isnan(sb)
    if a_nan != b_nan:
        return a_nan
    if not a_nan and sa != sb:
        return sa > sb
    return ia < ib                             # equal scores (-0.0 and 0.0 among them), or both NaN


def sort_total(cands):
    """[(index, score)] in the total order: insertion sort, a plain loop."""
    out = []
    for j, s in cands:
        at = len(out)
        while at > 0 and before(s, j, out[at - 1][1], out[at - 1][0]):
            at -= 1
        out.insert(at, (j, s))
    return out


def topk_of_sorted(rows, k):
    """(scores (B, k) fp64, indices (B, k) int64, n_candidates (B,)) of per-row candidate lists [(index, score)] in the total order."""
    B = len(rows)
    scores, indices = np.full((B, k), -np.inf), np.full((B, k), -1, dtype=np.int64)
    for i in range(B):
        for r, (j, s) in enumerate(rows[i][:k]):
            scores[i, r], indices[i, r] = s, j
    return scores, indices, np.array([len(c) for c in rows], dtype=np.int64)


def topk_of_cands(cands, k):
    """The same of unordered lists."""
    return topk_of_sorted([sort_total(c) for c in cands], k)


def topk_oracle(ref, k):
    """The oracle on a ranks_oracle result."""
    return topk_of_cands(ref['cands'], k)


def composition_topk(query, item, extra_item, k, item_ids=None, log_q=None, temperature=1.0, mask=None, extra_item_ids=None,
                     extra_log_q=None, extra_mask=None, remove_accidental_hits=True, in_batch_candidates=True):
    """The torch restatement a user writes without the fused kernel, in the dtype of `query`: cat + (B, B + N) logits + masked_fill + topk.
    (scores, indices, n_candidates, logits): slots past a row's candidates are (-inf, -1), as are the rows that do not take part."""
    import torch
    B, N = query.shape[0], extra_item.shape[0]
    s = query @ torch.cat([item, extra_item]).T / temperature
    if log_q is not None:
        s = s - torch.cat([log_q.reshape(-1), extra_log_q.reshape(-1)]).reshape(1, -1).to(s.dtype)
    eye = torch.cat([torch.eye(B, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)], dim=1)
    on = torch.ones(B, dtype=torch.bool) if mask is None else mask.reshape(-1) != 0
    xon = torch.ones(N, dtype=torch.bool) if extra_mask is None else extra_mask.reshape(-1) != 0
    keep = torch.cat([on, xon])[None, :].expand(B, B + N) & ~eye & on[:, None]
    if item_ids is not None and remove_accidental_hits:
        keep = keep & (torch.cat([item_ids.reshape(-1), extra_item_ids.reshape(-1)])[None, :] != item_ids.reshape(-1)[:, None])
    if not in_batch_candidates:
        keep = keep & torch.cat([torch.zeros(B, dtype=torch.bool), torch.ones(N, dtype=torch.bool)])[None, :]
    kk = min(k, B + N)
    top_s, top_i = torch.topk(s.masked_fill(~keep, float('-inf')), kk, dim=1)
    n_cand = keep.sum(1)
    live = torch.arange(kk)[None, :] < n_cand[:, None]                 # a kept -inf logit sorts with the removed ones: none in these tests
    scores = torch.full((B, k), float('-inf'), dtype=s.dtype)
    indices = torch.full((B, k), -1, dtype=torch.int64)
    scores[:, :kk] = torch.where(live, top_s, scores[:, :kk])
    indices[:, :kk] = torch.where(live, top_i, indices[:, :kk])
    return scores, indices, n_cand, s


def composition_of(case, k, dtype, in_batch_candidates=True):
    import torch
    t = lambda a, d=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(d) if d else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return composition_topk(t(case['query'], dtype), t(case['item'], dtype), t(case['extra_item'], dtype), k, t(case['item_ids']),
                            t(case['log_q'], dtype), case['temperature'], t(case['mask']), t(case['extra_item_ids']),
                            t(case['extra_log_q'], dtype), t(case['extra_mask']), in_batch_candidates=in_batch_candidates)


def check_float_regime(scores, indices, n_candidates, ref, k):
    """The float-regime contract on fp32 results against the fp64 candidate lists of `ref`, every taking-part row, none left out.
    Returns the worst observed fraction of (the per-logit bound, the exclusion bound)."""
    worst_s, worst_x = 0.0, 0.0
    assert np.array_equal(n_candidates, ref['n_candidates'])
    for i in range(len(ref['cands'])):
        if not ref['on'][i]:
            assert (indices[i] == -1).all() and np.isneginf(scores[i]).all() and n_candidates[i] == 0, 'row %d takes no part' % i
            continue
        exact = dict(ref['cands'][i])
        c = len(exact)
        live = min(k, c)
        assert (indices[i, :live] >= 0).all() and (indices[i, live:] == -1).all() and np.isneginf(scores[i, live:]).all(), 'row %d' % i
        idx = [int(j) for j in indices[i, :live]]
        assert len(set(idx)) == live and all(j in exact for j in idx), 'row %d: indices outside C\'(i) or repeated' % i
        for r, j in enumerate(idx):
            frac = abs(float(scores[i, r]) - exact[j]) / (LOGIT * max(1.0, abs(exact[j])))
            worst_s = max(worst_s, frac)
            assert frac <= 1.0, 'row %d slot %d: score off by %.3f of the bound' % (i, r, frac)
            if r > 0:
                assert before(float(scores[i, r - 1]), idx[r - 1], float(scores[i, r]), j), 'row %d: slots %d, %d out of order' % (i, r - 1, r)
        if live < c:
            last = float(scores[i, live - 1])
            kept = set(idx)
            for j, s in exact.items():
                if j not in kept:
                    frac = (s - last) / (GUARD * max(1.0, abs(s), abs(last)))
                    worst_x = max(worst_x, frac)
                    assert frac <= 1.0, 'row %d: candidate %d left out, %.3f of the bound above the last kept' % (i, j, frac)
    return worst_s, worst_x


@functools.lru_cache(maxsize=None)
def exact_sorted(B, N, D, config, in_batch_candidates=True):
    """(case, rank oracle, the candidate lists in the total order) of one exact-regime shape; computed once, shared, left unchanged."""
    case, ref = exact_ref(B, N, D, config, in_batch_candidates)
    return case, ref, [sort_total(c) for c in ref['cands']]

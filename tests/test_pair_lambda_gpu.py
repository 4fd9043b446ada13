"""GPU parity of the NDCG (LambdaRank) pair weight on the fused pairwise loss, of `ndcg_rank_terms` and of `in_batch_ndcg`
(csrc/pairwise_lambda.hip) against the dense fp64 oracle tests/_lambda_oracle.py, which restates the definitions and is pinned on the CPU in
tests/test_pair_lambda_cpu.py.

Bounds.  Pre-pass: positions exact (float32 compares, integer adds); discount, gain and inv_idcg within 1e-6 relative, the NDCG mean within
1e-6 absolute, the list count exact -- the terms are products of two correctly rounded float32 factors (2**-24 each) and the sums are fp64.
Loss: the project's own, as tests/test_pair_weight_table_gpu.py -- pair count exact, loss within 1e-5 * max(1, |ref|), gradient within
1e-5 * max|ref grad|.

Scores are round(N(0, 1) * 256) / 256, so the large groups are full of ties.  Hinge cases run with margin = m + 2**-10 and power-of-two
factors, and each asserts on the CPU, from the fp64 values alone, that no candidate lies within 2**-10 of the kink.  Wherever the fused route
is claimed, the module's `pair_indices` (the door to the general route) is patched to raise."""
import functools

import numpy as np
import pytest
import torch

import _lambda_oracle as O
from _pair_lists_oracle import no_general_route as _no_general_route

pytestmark = pytest.mark.gpu

RTOL = 1e-5
NAN = float('nan')
LOSSES = ('bpr', 'hinge', 'squared_hinge', 'margin_bpr')
BATCHES = ('b1', 'b2', 'b64', 'b1000', 'b2900')
HAND = ('equal', 'masked', 'single', 'zeros')


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _ndcg():
    from rec_now_amd.rec_block import ndcg
    return ndcg


def _t(a):
    return torch.from_numpy(np.array(a))         # a copy: the shared batches and references stay as they are


def _get(name):
    return O.hand_made(name[5:]) if name.startswith('hand_') else O.batch(name)


def _dev_groups(g, dev):
    return [_t(t).to(dev) for t in g] if isinstance(g, (list, tuple)) else _t(g).to(dev)


def _groups_of(g, variant):
    if variant == 'list':
        return [g, O.second_groups(g.size)]
    if variant == 'i64':
        return g.astype(np.int64) * 3000000007 - 5            # ids that need all 64 bits; same partition
    return g


# ---- pre-pass and metric -------------------------------------------------------------------------------------------------------------------
_TERMS = {}


def _terms(name, use_mask, gain, topn):
    key = (name, use_mask, gain, topn)
    if key not in _TERMS:
        g, s, y, mask = _get(name)
        _TERMS[key] = O.rank_terms(s, y, g, mask if use_mask else None, gain, topn)
    return _TERMS[key]


def _rel_ok(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if ref.size else 0.0
    print('%s: worst relative error %.3g' % (what, worst if np.isfinite(worst) else -1.0))
    assert (err <= 1e-6 * np.abs(ref)).all(), what                 # a reference of exactly 0 (no position, cut off, IDCG = 0) must be exactly 0


OPTIONS = [('exp2', None), ('exp2', 1), ('exp2', 5), ('linear', 5), ('linear', 5000), ('linear', None)]       # 5000: beyond every list


# every batch with its mask; the random ones without it as well (the hand-made lists are defined with theirs)
@pytest.mark.parametrize('name,use_mask', [(b, True) for b in BATCHES + tuple('hand_' + h for h in HAND)] + [(b, False) for b in BATCHES])
def test_rank_terms_and_metric(dev, name, use_mask):
    N = _ndcg()
    g, s, y, mask = _get(name)
    gd, sd, yd = _t(g).to(dev), _t(s).to(dev), _t(y).to(dev)
    md = _t(mask).to(dev) if use_mask else None
    seg = _mod().group_rows(gd)
    for gain, topn in OPTIONS:
        ref = _terms(name, use_mask, gain, topn)
        got = N.ndcg_rank_terms(sd, yd, gd, mask=md, gain=gain, topn=topn)
        assert got.rank.dtype == torch.int32 and got.rank.shape == (g.size,)
        assert np.array_equal(got.rank.cpu().numpy().astype(np.int64), ref.rank)
        _rel_ok(got.discount.cpu().numpy(), ref.discount, 'discount')
        _rel_ok(got.gain.cpu().numpy(), ref.gain, 'gain')
        _rel_ok(got.inv_idcg.cpu().numpy(), ref.inv_idcg, 'inv_idcg')
        mean, n_lists = N.in_batch_ndcg(sd, yd, None, mask=md, gain=gain, topn=topn, segments=seg)
        assert mean.dim() == 0 and n_lists.dim() == 0 and not mean.requires_grad
        print('%s %s topn %s: NDCG %.9g (ref %.9g) over %d lists (ref %d)' % (name, gain, topn, mean.item(), ref.ndcg_mean, n_lists.item(), ref.n_lists))
        assert n_lists.item() == ref.n_lists
        assert abs(mean.item() - ref.ndcg_mean) <= 1e-6
    if name.startswith('hand_'):
        first = g == 0
        ref = _terms(name, use_mask, 'exp2', None)
        if name[5:] in ('masked', 'zeros'):
            assert ref.n_lists == 2 and (ref.inv_idcg[first] == 0).all()
        if name[5:] == 'equal':
            rows = np.flatnonzero(first & mask)
            assert ref.rank[rows].tolist() == list(range(rows.size))          # the row-index rule
        if name[5:] == 'single':
            assert sorted(ref.rank[first].tolist()) == [-1] * 39 + [0]


def test_positions_of_each_list_form_a_permutation(dev):
    N = _ndcg()
    g, s, y, mask = O.batch('b2900')
    got = N.ndcg_rank_terms(_t(s).to(dev), _t(y).to(dev), _t(g).to(dev), mask=_t(mask).to(dev))
    rank = got.rank.cpu().numpy()
    assert (rank[~mask] == -1).all()
    for v in np.unique(g):
        rows = (g == v) & mask
        assert np.array_equal(np.sort(rank[rows]), np.arange(rows.sum()))


def test_all_lists_without_gain(dev):
    """Every label 0: no list has a positive IDCG -- the metric is 0 over 0 lists and the weighted loss is exactly 0 while the pairs count."""
    M, N = _mod(), _ndcg()
    g, s, _, mask = O.batch('b1000')
    y = np.zeros(g.size, dtype=np.float32)
    mean, n_lists = N.in_batch_ndcg(_t(s).to(dev), _t(y).to(dev), _t(g).to(dev), mask=_t(mask).to(dev))
    assert mean.item() == 0.0 and n_lists.item() == 0
    table = M.LabelPairWeightTable(O.LEVELS, O.w_sym)
    loss, n_pair, grad = _run(M, dev, g, s, y, mask, 0.0, False, label_pair_to_weight_func=table, lambda_weight=N.NDCGLambdaWeight())
    assert n_pair > 0 and loss == 0.0 and np.array_equal(grad, np.zeros_like(grad))


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------
def _pairloss(M, kind, margin, factor, reduce_mean=True):
    if kind == 'bpr':
        return functools.partial(M.bpr_loss_func, factor=factor, reduce_mean=reduce_mean)
    f = {'hinge': M.hinge_loss_func, 'squared_hinge': M.squared_hinge_loss_func, 'margin_bpr': M.margin_bpr_loss_func}[kind]
    return functools.partial(f, margin=margin, factor=factor, reduce_mean=reduce_mean)


def _options(kind, m, factor):
    """margin and factor of a case: the hinge kind sits half a grid step off every kink and takes power-of-two factors only."""
    if kind == 'hinge':
        assert factor in (1.0, 0.5, 2.0)
        return m + O.KINK, factor
    return m, factor


def _rule(M, rule):
    """(what pairwise_loss gets, what the oracle gets)"""
    if rule == 'default':
        return None, None
    return M.LabelPairWeightTable(O.LEVELS, O.w_sym), O.w_sym


_ORACLES = {}


def _oracle(batch_key, g, s, y, mask, kind, margin, factor, wf, power, wrong, lam, reduce_mean=True):
    """(loss, n_pair, gradient) of the dense fp64 formulation; computed once per distinct case (batch_key names g, s, y and mask)."""
    key = (batch_key, mask is not None, kind, margin, factor, None if wf is None else wf.__name__, power, wrong, lam, reduce_mean)
    if batch_key is not None and key in _ORACLES:
        return _ORACLES[key]
    s64 = _t(s).double().requires_grad_(True)
    rloss, rn = O.pairwise_loss(s64, y, g, O.ref_loss(kind, margin, factor, reduce_mean), wrong, power, mask, wf, lam)
    if rn:
        rloss.backward()
    grad = s64.grad.numpy() if s64.grad is not None else np.zeros(s.size)
    out = (rloss.item(), rn, grad)
    out[2].setflags(write=False)
    if batch_key is not None:
        _ORACLES[key] = out
    return out


def _run(M, dev, g, s, y, mask, power, wrong, upstream=None, **kw):
    sd = _t(s).to(dev).requires_grad_(True)
    loss, n_pair = M.pairwise_loss(sd, _t(y).to(dev), _dev_groups(g, dev), only_use_wrong_order_pair=wrong, return_num_pair=True,
                                   click_occurance_power=power, mask=None if mask is None else _t(mask).to(dev), **kw)
    (loss if upstream is None else upstream * loss).backward()
    return loss.item(), n_pair.item(), sd.grad.cpu().numpy()


def _check(got, want, grad_scale=1.0):
    loss, n_pair, grad = got
    rloss, rn, rgrad = want
    rgrad = rgrad * grad_scale
    gerr = np.abs(grad - rgrad).max() if grad.size else 0.0
    scale = max(np.abs(rgrad).max(), 1e-12) if grad.size else 1.0
    print('n_pair %d (ref %d)  loss %.9g (ref %.9g, err %.3g)  grad err %.3g of max %.3g' % (n_pair, rn, loss, rloss, abs(loss - rloss), gerr, scale))
    assert n_pair == rn                                               # integer path: exact, and untouched by the weight
    assert abs(loss - rloss) <= RTOL * max(1.0, abs(rloss))
    assert gerr <= RTOL * scale


# the four pair losses x {default rule, symmetric table} on the two large batches; the small and the hand-made batches; then one case each of
# the wrong-order rule, the occurrence weight, a second group tensor, int64 ids, the raw sum, topn and the linear gain
CASES = [
    # loss, batch, rule, power, wrong order, mask, m, factor, groups, gain, topn, reduce_mean
] + [(k, b, r, 0.0, False, True, 1.0, 1.0, 'f32', 'exp2', None, True) for b in ('b1000', 'b2900') for k in LOSSES for r in ('default', 'sym')] + [
    ('bpr', 'b1', 'default', 0.0, False, False, 0.0, 1.0, 'f32', 'exp2', None, True),
    ('hinge', 'b1', 'sym', -0.5, False, True, 1.0, 1.0, 'f32', 'exp2', None, True),
    ('bpr', 'b2', 'default', 0.0, False, True, 0.0, 1.0, 'f32', 'exp2', None, True),
    ('squared_hinge', 'b2', 'sym', 0.0, False, False, 1.0, 0.7, 'f32', 'linear', None, True),
    ('margin_bpr', 'b64', 'default', 0.0, False, True, 0.3, 1.0, 'f32', 'exp2', None, True),
    ('hinge', 'b64', 'sym', 0.0, False, False, 0.5, 2.0, 'f32', 'exp2', 5, True),
    ('bpr', 'hand_equal', 'sym', 0.0, False, True, 0.0, 1.0, 'f32', 'exp2', None, True),
    ('hinge', 'hand_masked', 'default', 0.0, False, True, 1.0, 1.0, 'f32', 'exp2', None, True),
    ('squared_hinge', 'hand_single', 'sym', -0.5, False, True, 1.0, 1.0, 'f32', 'exp2', None, True),
    ('margin_bpr', 'hand_zeros', 'sym', 0.0, False, True, 1.0, 1.0, 'f32', 'exp2', None, True),
    ('bpr', 'b1000', 'default', 0.0, True, True, 0.0, 1.0, 'f32', 'exp2', None, True),
    ('hinge', 'b2900', 'sym', 0.0, True, True, 1.0, 1.0, 'f32', 'exp2', None, True),
    ('bpr', 'b1000', 'sym', -0.5, False, True, 0.0, 0.7, 'f32', 'exp2', None, True),
    ('squared_hinge', 'b2900', 'default', -0.5, False, False, 0.5, 1.0, 'f32', 'exp2', None, True),
    ('margin_bpr', 'b1000', 'sym', 0.0, False, True, 1.0, 1.0, 'list', 'exp2', None, True),
    ('bpr', 'b1000', 'default', -0.5, False, True, 0.0, 1.0, 'i64', 'exp2', None, True),
    ('hinge', 'b1000', 'default', 1.0, False, True, 1.0, 0.5, 'f32', 'exp2', None, False),
    ('bpr', 'b2900', 'sym', 0.0, False, True, 0.0, 1.0, 'f32', 'exp2', 5, True),
    ('squared_hinge', 'b1000', 'default', 0.0, False, True, 1.0, 1.0, 'f32', 'exp2', 1, True),
    ('margin_bpr', 'b2900', 'default', 0.0, False, True, 0.3, 1.0, 'f32', 'linear', None, True),
]


@pytest.mark.parametrize('kind,name,rule,power,wrong,use_mask,m,factor,variant,gain,topn,reduce_mean', CASES)
def test_lambda_route_vs_oracle(dev, monkeypatch, kind, name, rule, power, wrong, use_mask, m, factor, variant, gain, topn, reduce_mean):
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _get(name)
    if not use_mask:
        mask = None
    g = _groups_of(g, variant)
    margin, factor = _options(kind, m, factor)
    if kind == 'hinge':
        O.assert_off_the_kink(g, s, margin, factor)
    table, wf = _rule(M, rule)
    got = _run(M, dev, g, s, y, mask, power, wrong, pairloss_func=_pairloss(M, kind, margin, factor, reduce_mean),
               label_pair_to_weight_func=table, lambda_weight=N.NDCGLambdaWeight(gain=gain, topn=topn))
    want = _oracle((name, variant), g, s, y, mask, kind, margin, factor, wf, power, wrong, (gain, topn), reduce_mean)
    _check(got, want)
    # the weight changes the value, never the pair set: the same call without it has the same count and another loss
    if name == 'b1000' and variant == 'f32':
        plain = _run(M, dev, g, s, y, mask, power, wrong, pairloss_func=_pairloss(M, kind, margin, factor, reduce_mean), label_pair_to_weight_func=table)
        assert plain[1] == got[1]
        assert abs(plain[0] - got[0]) > 1e-3 * abs(plain[0])


def test_the_default_pair_loss_takes_the_keyword(dev, monkeypatch):
    """pairwise_loss(..., lambda_weight=w) with nothing else: BPR, factor 1, mean -- and not the unweighted loss."""
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = O.batch('b1000')
    got = _run(M, dev, g, s, y, mask, 0.0, False, lambda_weight=N.NDCGLambdaWeight())
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, 'bpr', 0.0, 1.0, None, 0.0, False, ('exp2', None)))
    sd = _t(s).to(dev)
    loss = M.pairwise_loss(sd, _t(y).to(dev), _t(g).to(dev), mask=_t(mask).to(dev), lambda_weight=N.NDCGLambdaWeight())
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and loss.item() == got[0]


def test_fused_entry_with_precomputed_segments(dev):
    M, N = _mod(), _ndcg()
    g, s, y, mask = O.batch('b1000')
    gd = _t(g).to(dev)
    sd = _t(s).to(dev).requires_grad_(True)
    lam = N.NDCGLambdaWeight(gain='linear', topn=5)
    table, wf = _rule(M, 'sym')
    margin, factor = _options('hinge', 0.5, 2.0)
    O.assert_off_the_kink(g, s, margin, factor)
    for kind, kw in (('bpr', {}), ('hinge', {'kind': 'hinge', 'margin': margin})):
        sd.grad = None
        loss, n_pair = M.pairwise_loss_fused(sd, _t(y).to(dev), None, click_occurance_power=-0.5, mask=_t(mask).to(dev), factor=factor,
                                             reduce_mean=False, segments=M.group_rows(gd), label_pair_weights=table, lambda_weight=lam, **kw)
        loss.backward()
        _check((loss.item(), n_pair.item(), sd.grad.cpu().numpy()),
               _oracle(('b1000', 'f32'), g, s, y, mask, kind, margin, factor, wf, -0.5, False, ('linear', 5), reduce_mean=False))
    loss, n_pair = M.pairwise_loss_fused(sd, _t(y).to(dev), gd, lambda_weight=lam, return_num_pair=False)
    assert n_pair is None and loss.dim() == 0


def test_upstream_gradient_scales_the_result(dev, monkeypatch):
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = O.batch('b1000')
    got = _run(M, dev, g, s, y, mask, 0.0, False, upstream=3.0, lambda_weight=N.NDCGLambdaWeight())
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, 'bpr', 0.0, 1.0, None, 0.0, False, ('exp2', None)), grad_scale=3.0)


def test_unknown_label_still_poisons(dev, monkeypatch):
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = O.batch('b1000')
    table, wf = _rule(M, 'sym')
    row = int(np.flatnonzero(mask)[10])
    y = y.copy()
    y[row] = 7.0
    for kind in ('bpr', 'squared_hinge'):
        loss, n_pair, grad = _run(M, dev, g, s, y, mask, -0.5, False, pairloss_func=_pairloss(M, kind, 1.0, 1.0), label_pair_to_weight_func=table,
                                  lambda_weight=N.NDCGLambdaWeight())
        assert np.isnan(loss) and np.isnan(grad).all()
    mask2 = mask.copy()
    mask2[row] = False                                            # the same row masked out: no effect, finite and equal to the oracle
    got = _run(M, dev, g, s, y, mask2, -0.5, False, label_pair_to_weight_func=table, lambda_weight=N.NDCGLambdaWeight())
    assert np.isfinite(got[0]) and np.isfinite(got[2]).all()
    _check(got, _oracle(None, g, s, y, mask2, 'bpr', 0.0, 1.0, wf, -0.5, False, ('exp2', None)))


def test_no_pairs(dev, monkeypatch):
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = O.batch('b1000')
    none = np.zeros(g.size, dtype=bool)
    for kind in LOSSES:
        loss, n_pair, grad = _run(M, dev, g, s, y, none, -0.5, False, pairloss_func=_pairloss(M, kind, 1.0, 1.0), lambda_weight=N.NDCGLambdaWeight())
        assert loss == 0.0 and n_pair == 0.0 and np.array_equal(grad, np.zeros_like(grad))


# ---- routing -------------------------------------------------------------------------------------------------------------------------------
def test_lambda_wrapped_loss_takes_the_general_route(dev, monkeypatch):
    """A pair loss inside a lambda goes through the pair list; the weight is formed there from ndcg_rank_terms and held to the same oracle."""
    M, N = _mod(), _ndcg()
    g, s, y, mask = O.batch('b1000')
    calls = []
    real = M.pair_indices

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(M, 'pair_indices', spy)
    lam = N.NDCGLambdaWeight(topn=5)
    got = _run(M, dev, g, s, y, mask, -0.5, False, pairloss_func=lambda p, n, w: M.bpr_loss_func(p, n, w, factor=0.7), lambda_weight=lam)
    assert calls
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, 'bpr', 0.0, 0.7, None, -0.5, False, ('exp2', 5)))
    # a plain weight function beside a fusable loss: the general route as well
    del calls[:]
    got = _run(M, dev, g, s, y, mask, 0.0, False, label_pair_to_weight_func=lambda a, b, **k: O.w_sym(a, b), lambda_weight=lam)
    assert calls
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, 'bpr', 0.0, 1.0, O.w_sym, 0.0, False, ('exp2', 5)))


# ---- repeatability -------------------------------------------------------------------------------------------------------------------------
def test_run_to_run_bit_identical(dev, monkeypatch):
    M, N = _mod(), _ndcg()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = O.batch('b2900')
    table, _ = _rule(M, 'sym')
    lam = N.NDCGLambdaWeight()
    for kind, t, power in (('bpr', table, -0.5), ('hinge', None, 0.0)):
        lf = _pairloss(M, kind, 0.5, 1.0)
        a = _run(M, dev, g, s, y, mask, power, False, pairloss_func=lf, label_pair_to_weight_func=t, lambda_weight=lam)
        b = _run(M, dev, g, s, y, mask, power, False, pairloss_func=lf, label_pair_to_weight_func=t, lambda_weight=lam)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
        assert a[1] == b[1]
        assert a[2].tobytes() == b[2].tobytes() and np.abs(a[2]).max() > 0
    sd, yd, gd = _t(s).to(dev), _t(y).to(dev), _t(g).to(dev)
    m1, n1 = N.in_batch_ndcg(sd, yd, gd)
    m2, n2 = N.in_batch_ndcg(sd, yd, gd)
    assert np.float32(m1.item()).tobytes() == np.float32(m2.item()).tobytes() and n1.item() == n2.item()


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments(dev):
    from rec_now_amd import _lib
    M = _mod()
    lib = _lib.load()
    g, s, y, mask = O.batch('b64')
    seg = M.group_rows(_t(g).to(dev))
    B = seg.B
    sd, yd = _t(s).to(dev), _t(y).to(dev)
    P, st = _lib.ptr, _lib.stream()
    EINVAL, EWORKSPACE = -1, -2                                 # RECNOW_EINVAL, RECNOW_EWORKSPACE of include/recnow.h
    assert lib.recnow_pair_lambda_workspace_bytes(B) > lib.recnow_pairwise_workspace_bytes(B)
    ws = _lib.workspace(lib.recnow_pair_lambda_workspace_bytes(B), dev)

    def terms(flags=0, gain=0, nbytes=None, scores=sd):
        return lib.recnow_pair_lambda_terms(P(scores), P(yd), None, P(seg.order), P(seg.seg_id), P(seg.seg_first), B, flags, gain, 0, None, None, None,
                                            None, None, None, None, None, P(ws), ws.numel() if nbytes is None else nbytes, st)
    assert terms() == 0
    assert terms(gain=2) == EINVAL and terms(gain=-1) == EINVAL
    assert terms(flags=1) == EINVAL and terms(flags=2) == EINVAL
    assert terms(scores=None) == EINVAL                         # nothing packed and nothing to pack from
    assert terms(nbytes=lib.recnow_pairwise_workspace_bytes(B)) == EWORKSPACE
    cnt_row = torch.empty(B, dtype=torch.int32, device=dev)
    cnt_super = torch.empty(B, dtype=torch.int64, device=dev)
    n_pair = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call('recnow_pair_count', P(sd), P(yd), None, P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), B, 1, P(cnt_row),
              P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
    assert terms(flags=256) == 0
    loss = torch.full((), 7.0, dtype=torch.float32, device=dev)
    dscores = torch.zeros(B, dtype=torch.float32, device=dev)

    def walk(flags=1 | 256, kind=3, margin=0.0, factor=1.0, nbytes=None, nB=B):
        return lib.recnow_pair_lambda_fwdbwd(P(seg.seg_id), P(seg.seg_first), P(seg.super_id), P(cnt_super), P(n_pair), nB, flags, kind, margin, 0,
                                             None, factor, 0.0, 1, P(loss), P(dscores), P(ws), ws.numel() if nbytes is None else nbytes, st)
    assert walk() == 0
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and loss.item() != 7.0
    assert walk(flags=1) == EINVAL                              # the members and the records must be those in the workspace
    assert walk(flags=256) == EINVAL                            # no table and no RECNOW_PAIR_LABEL_GT
    assert walk(flags=1 | 256 | 8) == EINVAL
    for kind in (0, 4, -1):
        assert walk(kind=kind) == EINVAL
    assert walk(margin=float('inf')) == EINVAL and walk(factor=NAN) == EINVAL
    assert walk(nbytes=lib.recnow_pairwise_workspace_bytes(B)) == EWORKSPACE
    assert walk(nB=0) == 0
    torch.cuda.synchronize()
    assert loss.item() == 0.0

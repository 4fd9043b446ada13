"""GPU parity of the fused pairwise loss with hinge_loss_func, squared_hinge_loss_func and margin_bpr_loss_func (csrc/pairwise_kind.hip) against
the dense fp64 oracle (oracle/dense_ref.pairwise_loss, torch autograd for the gradient).  The oracle is handed an fp64 restatement of the pair
loss written here, never the function under test, and the ORIGINAL weight function where a LabelPairWeightTable is used.  Bounds as
tests/test_pair_weight_table_gpu.py: pair count exact, loss within 1e-5 * max(1, |ref|), gradient within 1e-5 * max|ref grad|.

Scores are round(N(0, 1) * 256) / 256.  The hinge kind runs with margin = m + 2**-10 and factors that are powers of two: every
u = margin - factor (s_i - s_j) is then an exact odd multiple of 2**-10 in fp32 and in fp64, so no candidate lies at or within rounding of the
kink (a single pair whose fp32 u had the other sign would flip a gradient term of size 1 / P, far above the bound).  Each hinge case asserts
that on the CPU from the fp64 values alone.

Wherever the fused route is claimed, the module's `pair_indices` (the door to the general route) is patched to raise."""
import functools

import numpy as np
import pytest
import torch

from _pair_lists_oracle import no_general_route as _no_general_route
import dense_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-5
LEVELS = [0.0, 1.0, 2.0, 3.0]
NAN = float('nan')
KINK = 2.0 ** -10
KINDS = ('hinge', 'squared_hinge', 'margin_bpr')


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _t(a):
    return torch.from_numpy(np.array(a))         # a copy: the shared batches and references stay as they are


def _func(M, kind):
    return {'hinge': M.hinge_loss_func, 'squared_hinge': M.squared_hinge_loss_func, 'margin_bpr': M.margin_bpr_loss_func}[kind]


# ---- the pair losses, restated in fp64 torch ---------------------------------------------------------------------------------------------
def _ref_loss(kind, margin, factor, reduce_mean=True):
    def loss(pos, neg, weights=None):
        u = margin - factor * (pos - neg)
        if kind == 'hinge':
            t = torch.relu(u)
        elif kind == 'squared_hinge':
            t = torch.relu(u) * torch.relu(u)
        else:
            t = torch.logaddexp(u, torch.zeros_like(u))       # softplus, smooth at u == 0 (relu + log1p(exp(-|u|)) has autograd derivative 0 there, not 1 / 2)
        n = t.numel()
        if weights is not None:
            t = t * weights
        return t.sum() / (n + 1e-10) if reduce_mean else t.sum()
    return loss


# ---- pair rules: None (label_i > label_j), and two tables with the weight functions the oracle sees ------------------------------------------
def _w_sym(a, b, **k):                       # both directions, tied labels are pairs
    return (a - b).abs() + 0.5


# explicit, asymmetric: zero, negative, NaN and positive entries, positive on part of the diagonal
W_EXPLICIT = [[0.5, 0.0, -1.0, NAN],
              [1.5, 0.0, 0.25, 0.0],
              [2.0, 0.75, 1.0, -0.5],
              [NAN, 3.0, 0.0, 0.0]]


def _w_explicit(a, b, **k):                  # the oracle's view: labels are the integers 0..3
    return torch.tensor(W_EXPLICIT, dtype=a.dtype)[a.long(), b.long()]


def _rule(M, rule):
    """(what pairwise_loss gets, what the oracle gets)"""
    if rule == 'default':
        return None, None
    if rule == 'sym':
        return M.LabelPairWeightTable(LEVELS, _w_sym), _w_sym
    return M.LabelPairWeightTable(LEVELS, weights=W_EXPLICIT), _w_explicit


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(name):
    """(groups, scores, labels, mask) as numpy; scores on the 1 / 256 grid, labels in {0, 1, 2, 3}, the mask keeps ~80 % of the rows."""
    if name in _BATCHES:
        return _BATCHES[name]
    seed = {'b1': 1, 'b2': 2, 'b64': 3, 'b1000': 4, 'b2900': 5}[name]
    rng = np.random.default_rng(seed)
    if name == 'b2900':
        # one group beyond PW_STAGE = 2048 (global-memory walk), one beyond PW_LONG = 512 (wave per row inside LDS), 200 rows in small groups
        groups = np.concatenate([np.zeros(2100), np.ones(600), rng.integers(2, 22, 200)]).astype(np.float32)
        rng.shuffle(groups)
    else:
        B, G = {'b1': (1, 1), 'b2': (2, 1), 'b64': (64, 4), 'b1000': (1000, 17)}[name]
        groups = rng.integers(0, G, B).astype(np.float32)
    B = groups.size
    scores = (np.round(rng.normal(size=B) * 256) / 256).astype(np.float32)
    labels = rng.integers(0, 4, B).astype(np.float32)
    mask = rng.random(B) < 0.8
    for a in (groups, scores, labels, mask):
        a.setflags(write=False)
    _BATCHES[name] = (groups, scores, labels, mask)
    return _BATCHES[name]


def _second_groups(B):
    g2 = np.random.default_rng(77).integers(0, 3, B).astype(np.float32)
    g2.setflags(write=False)
    return g2


def _as_list(g):
    return list(g) if isinstance(g, (list, tuple)) else [g]


def _assert_off_the_kink(g, s, margin, factor):
    """From the fp64 values alone: no same-group candidate (i, j), i != j, has |margin - factor (s_i - s_j)| below 2**-10."""
    gl = _as_list(g)
    if gl[0].size < 2:
        return
    same = np.ones((gl[0].size, gl[0].size), dtype=bool)
    for t in gl:
        same &= t.reshape(-1, 1) == t.reshape(1, -1)
    np.fill_diagonal(same, False)
    if not same.any():
        return
    s64 = s.astype(np.float64)
    u = margin - factor * (s64.reshape(-1, 1) - s64.reshape(1, -1))
    assert np.abs(u[same]).min() >= KINK


_ORACLES = {}


def _oracle(batch_key, g, s, y, mask, kind, margin, factor, wf, power, wrong, reduce_mean=True):
    """(loss, n_pair, gradient) of the dense fp64 formulation; computed once per distinct case (batch_key names g, s, y and mask)."""
    key = (batch_key, mask is not None, kind, margin, factor, None if wf is None else wf.__name__, power, wrong, reduce_mean)
    if batch_key is not None and key in _ORACLES:
        return _ORACLES[key]
    s64 = _t(s).double().requires_grad_(True)
    gt = [_t(t) for t in g] if isinstance(g, (list, tuple)) else _t(g)
    rloss, rn = R.pairwise_loss(s64, _t(y).double(), gt, _ref_loss(kind, margin, factor, reduce_mean),
                                only_use_wrong_order_pair=wrong, return_num_pair=True, click_occurance_power=power,
                                mask=None if mask is None else _t(mask), label_pair_to_weight_func=wf)
    rloss.backward()
    out = (rloss.item(), rn, s64.grad.numpy())
    out[2].setflags(write=False)
    if batch_key is not None:
        _ORACLES[key] = out
    return out


def _run(M, dev, g, s, y, mask, power, wrong, upstream=None, **kw):
    sd = _t(s).to(dev).requires_grad_(True)
    gd = [_t(t).to(dev) for t in g] if isinstance(g, (list, tuple)) else _t(g).to(dev)
    loss, n_pair = M.pairwise_loss(sd, _t(y).to(dev), gd, only_use_wrong_order_pair=wrong, return_num_pair=True,
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
    assert n_pair == rn                                               # integer path: exact
    assert abs(loss - rloss) <= RTOL * max(1.0, abs(rloss))
    assert gerr <= RTOL * scale


def _options(kind, m, factor):
    """margin and factor of a case: the hinge kind sits half a grid step off every kink and takes power-of-two factors only."""
    if kind == 'hinge':
        assert factor in (1.0, 0.5, 2.0)
        return m + KINK, factor
    return m, factor


# ---- parity: a covering list.  Every kind meets every batch; every rule meets b1000 and b2900 for every kind; powers 0 / -0.5 / 1, the
# wrong-order rule, the mask, a list of two group tensors and int64 ids are spread over it. ----------------------------------------------------
CASES = [
    # kind, batch, rule, power, wrong order, mask, m, factor, groups
    ('hinge', 'b1', 'default', 0.0, False, False, 1.0, 1.0, 'f32'),
    ('squared_hinge', 'b1', 'sym', -0.5, False, True, 1.0, 0.7, 'f32'),
    ('margin_bpr', 'b1', 'explicit', 1.0, True, False, 0.3, 1.0, 'f32'),
    ('hinge', 'b2', 'sym', -0.5, False, False, 0.5, 2.0, 'f32'),
    ('squared_hinge', 'b2', 'default', 0.0, True, True, 1.0, 1.0, 'f32'),
    ('margin_bpr', 'b2', 'sym', 0.0, False, False, 1.0, 0.7, 'f32'),
    ('hinge', 'b64', 'explicit', 1.0, False, True, 1.0, 0.5, 'f32'),
    ('squared_hinge', 'b64', 'default', -0.5, False, False, 0.5, 1.0, 'f32'),
    ('margin_bpr', 'b64', 'sym', 0.0, True, True, 0.0, 1.0, 'f32'),
    ('hinge', 'b1000', 'default', 0.0, False, True, 1.0, 1.0, 'f32'),
    ('hinge', 'b1000', 'sym', -0.5, True, True, 0.5, 2.0, 'f32'),
    ('hinge', 'b1000', 'explicit', 1.0, False, False, 1.0, 0.5, 'f32'),
    ('squared_hinge', 'b1000', 'default', 1.0, True, False, 1.0, 0.7, 'f32'),
    ('squared_hinge', 'b1000', 'sym', 0.0, False, True, 0.5, 1.0, 'f32'),
    ('squared_hinge', 'b1000', 'explicit', -0.5, False, True, 1.0, 1.0, 'f32'),
    ('margin_bpr', 'b1000', 'default', -0.5, False, True, 1.0, 0.7, 'f32'),
    ('margin_bpr', 'b1000', 'sym', 1.0, False, False, 0.3, 1.0, 'f32'),
    ('margin_bpr', 'b1000', 'explicit', 0.0, True, True, 1.0, 0.7, 'f32'),
    ('hinge', 'b2900', 'default', -0.5, True, True, 1.0, 1.0, 'f32'),
    ('hinge', 'b2900', 'sym', 0.0, False, False, 1.0, 1.0, 'f32'),
    ('hinge', 'b2900', 'explicit', -0.5, False, True, 0.5, 0.5, 'f32'),
    ('squared_hinge', 'b2900', 'default', 0.0, False, True, 1.0, 1.0, 'f32'),
    ('squared_hinge', 'b2900', 'sym', 1.0, False, False, 1.0, 0.7, 'f32'),
    ('squared_hinge', 'b2900', 'explicit', -0.5, True, True, 0.5, 1.0, 'f32'),
    ('margin_bpr', 'b2900', 'default', 1.0, False, False, 1.0, 1.0, 'f32'),
    ('margin_bpr', 'b2900', 'sym', -0.5, False, True, 1.0, 0.7, 'f32'),
    ('margin_bpr', 'b2900', 'explicit', 0.0, True, False, 0.3, 0.7, 'f32'),
    ('hinge', 'b1000', 'sym', -0.5, False, True, 1.0, 1.0, 'list'),
    ('squared_hinge', 'b2900', 'default', -0.5, False, True, 1.0, 1.0, 'list'),
    ('margin_bpr', 'b1000', 'explicit', 1.0, False, True, 1.0, 0.7, 'list'),
    ('hinge', 'b1000', 'default', -0.5, False, True, 1.0, 2.0, 'i64'),
    ('margin_bpr', 'b2900', 'sym', 0.0, False, True, 1.0, 1.0, 'i64'),
]


def _groups_of(g, variant):
    if variant == 'list':
        return [g, _second_groups(g.size)]
    if variant == 'i64':
        return g.astype(np.int64) * 3000000007 - 5            # ids that need all 64 bits; same partition
    return g


@pytest.mark.parametrize('kind,batch,rule,power,wrong,use_mask,m,factor,variant', CASES)
def test_kind_route_vs_oracle(dev, monkeypatch, kind, batch, rule, power, wrong, use_mask, m, factor, variant):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch(batch)
    if not use_mask:
        mask = None
    elif batch in ('b1', 'b2'):
        mask = np.ones(g.size, dtype=bool)
    g = _groups_of(g, variant)
    margin, factor = _options(kind, m, factor)
    if kind == 'hinge':
        _assert_off_the_kink(g, s, margin, factor)
    table, wf = _rule(M, rule)
    got = _run(M, dev, g, s, y, mask, power, wrong, pairloss_func=functools.partial(_func(M, kind), margin=margin, factor=factor),
               label_pair_to_weight_func=table)
    _check(got, _oracle((batch, variant), g, s, y, mask, kind, margin, factor, wf, power, wrong))


@pytest.mark.parametrize('kind', KINDS)
def test_the_functions_themselves_use_their_defaults(dev, monkeypatch, kind):
    """pairloss_func=F with nothing bound: margin 1, factor 1, mean.  With margin exactly 1 candidates of the hinge kinds do sit ON the kink
    (u == 0.0 exactly, in fp32 as in fp64: every u is a multiple of 1 / 256), never within rounding of it: the subgradient there is 0 on
    both sides, as torch.relu's."""
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b1000')
    got = _run(M, dev, g, s, y, mask, 0.0, False, pairloss_func=_func(M, kind))
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, kind, 1.0, 1.0, None, 0.0, False))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rule', ['default', 'sym'])
def test_options_through_functools_partial(dev, monkeypatch, kind, rule):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b1000')
    margin, factor = _options(kind, 0.25, 0.5)
    if kind == 'hinge':
        _assert_off_the_kink(g, s, margin, factor)
    table, wf = _rule(M, rule)
    lf = functools.partial(_func(M, kind), reduce_mean=False, factor=factor, margin=margin)
    got = _run(M, dev, g, s, y, mask, -0.5, False, pairloss_func=lf, label_pair_to_weight_func=table)
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, kind, margin, factor, wf, -0.5, False, reduce_mean=False))


@pytest.mark.parametrize('kind', KINDS)
def test_fused_entry_with_precomputed_segments(dev, kind):
    M = _mod()
    g, s, y, mask = _batch('b1000')
    margin, factor = _options(kind, 0.5, 2.0)
    if kind == 'hinge':
        _assert_off_the_kink(g, s, margin, factor)
    table, wf = _rule(M, 'explicit')
    gd = _t(g).to(dev)
    sd = _t(s).to(dev).requires_grad_(True)
    for t, f in ((table, wf), (None, None)):
        sd.grad = None
        loss, n_pair = M.pairwise_loss_fused(sd, _t(y).to(dev), None, click_occurance_power=-0.5, mask=_t(mask).to(dev),
                                             factor=factor, reduce_mean=False, segments=M.group_rows(gd), label_pair_weights=t, kind=kind,
                                             margin=margin)
        loss.backward()
        _check((loss.item(), n_pair.item(), sd.grad.cpu().numpy()),
               _oracle(('b1000', 'f32'), g, s, y, mask, kind, margin, factor, f, -0.5, False, reduce_mean=False))
    loss, n_pair = M.pairwise_loss_fused(sd, _t(y).to(dev), gd, kind=kind, margin=margin, return_num_pair=False)
    assert n_pair is None and loss.dim() == 0


@pytest.mark.parametrize('kind', KINDS)
def test_upstream_gradient_scales_the_result(dev, monkeypatch, kind):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b1000')
    margin, factor = _options(kind, 1.0, 1.0)
    if kind == 'hinge':
        _assert_off_the_kink(g, s, margin, factor)
    table, wf = _rule(M, 'sym')
    got = _run(M, dev, g, s, y, mask, 0.0, False, upstream=3.0, pairloss_func=functools.partial(_func(M, kind), margin=margin),
               label_pair_to_weight_func=table)
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, kind, margin, factor, wf, 0.0, False), grad_scale=3.0)


def test_fully_satisfied_hinge(dev, monkeypatch):
    """scores = 10 * label, margin 1, the default rule: every pair has u <= 1 - 10 < 0 -- pairs exist, the loss is exactly 0.0 and so is every
    gradient entry (the mean still divides by the number of pairs)."""
    M = _mod()
    _no_general_route(monkeypatch, M)
    for batch in ('b1000', 'b2900'):
        g, _, y, mask = _batch(batch)
        s = (10.0 * y).astype(np.float32)
        for kind in ('hinge', 'squared_hinge'):
            for power in (0.0, -0.5):
                loss, n_pair, grad = _run(M, dev, g, s, y, mask, power, False, pairloss_func=_func(M, kind))
                assert n_pair > 0
                assert loss == 0.0
                assert np.array_equal(grad, np.zeros_like(grad))


@pytest.mark.parametrize('kind', KINDS)
def test_no_pairs(dev, monkeypatch, kind):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b1000')
    dead = M.LabelPairWeightTable(LEVELS, weights=[[0.0, -1.0, NAN, 0.0], [-0.5, 0.0, 0.0, NAN], [0.0, 0.0, -2.0, 0.0], [NAN, 0.0, 0.0, 0.0]])
    live, _ = _rule(M, 'sym')
    none = np.zeros(g.size, dtype=bool)
    for t, m in ((dead, mask), (dead, None), (live, none), (None, none)):
        for power in (0.0, -0.5):
            loss, n_pair, grad = _run(M, dev, g, s, y, m, power, False, pairloss_func=_func(M, kind), label_pair_to_weight_func=t)
            assert loss == 0.0 and n_pair == 0.0
            assert np.array_equal(grad, np.zeros_like(grad))


@pytest.mark.parametrize('kind', KINDS)
def test_unknown_label(dev, monkeypatch, kind):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b1000')
    table, wf = _rule(M, 'sym')
    margin, factor = _options(kind, 1.0, 1.0)
    lf = functools.partial(_func(M, kind), margin=margin)
    row = int(np.flatnonzero(mask)[10])
    y = y.copy()
    y[row] = 7.0
    for m, power in ((mask, 0.0), (None, -0.5)):
        loss, n_pair, grad = _run(M, dev, g, s, y, m, power, False, pairloss_func=lf, label_pair_to_weight_func=table)
        assert np.isnan(loss)
        assert np.isnan(grad).all()
    # the same row masked out: no effect, finite and equal to the oracle
    mask2 = mask.copy()
    mask2[row] = False
    if kind == 'hinge':
        _assert_off_the_kink(g, s, margin, factor)
    got = _run(M, dev, g, s, y, mask2, -0.5, False, pairloss_func=lf, label_pair_to_weight_func=table)
    assert np.isfinite(got[0]) and np.isfinite(got[2]).all()
    _check(got, _oracle(None, g, s, y, mask2, kind, margin, factor, wf, -0.5, False))
    # without a table every label is just a number: the default rule never raises the flag
    got = _run(M, dev, g, s, y, mask, 0.0, False, pairloss_func=lf)
    assert np.isfinite(got[0]) and np.isfinite(got[2]).all()


@pytest.mark.parametrize('kind', KINDS)
def test_run_to_run_bit_identical(dev, monkeypatch, kind):
    M = _mod()
    _no_general_route(monkeypatch, M)
    g, s, y, mask = _batch('b2900')
    table, _ = _rule(M, 'sym')
    lf = functools.partial(_func(M, kind), margin=0.5)
    for t, power in ((table, -0.5), (None, 0.0)):
        a = _run(M, dev, g, s, y, None, power, False, pairloss_func=lf, label_pair_to_weight_func=t)
        b = _run(M, dev, g, s, y, None, power, False, pairloss_func=lf, label_pair_to_weight_func=t)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
        assert a[1] == b[1]
        assert a[2].tobytes() == b[2].tobytes()


def test_no_memory_proportional_to_the_pairs(dev):
    """B 2900 with the symmetric table and no mask: every ordered pair inside a group is a pair, P > 4 million (8 bytes per pair alone: > 35 MB).
    The fused hinge route's peak allocation across forward + backward stays below 16 pairwise workspaces; the general route, given the same
    function wrapped in a lambda, agrees within the bound."""
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, _ = _batch('b2900')
    table, _ = _rule(M, 'sym')
    margin = 1.0 + KINK
    _assert_off_the_kink(g, s, margin, 1.0)
    lf = functools.partial(M.hinge_loss_func, margin=margin)
    gd, yd = _t(g).to(dev), _t(y).to(dev)
    sd = _t(s).to(dev).requires_grad_(True)
    M.pairwise_loss(sd, yd, gd, pairloss_func=lf, label_pair_to_weight_func=table)              # (uploads the table: 80 bytes that stay)
    sd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, n_pair = M.pairwise_loss(sd, yd, gd, pairloss_func=lf, return_num_pair=True, label_pair_to_weight_func=table)
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    bound = 16 * _lib.load().recnow_pairwise_workspace_bytes(g.size)
    print('pairs %d  peak growth %d bytes  bound %d bytes' % (n_pair.item(), growth, bound))
    assert n_pair.item() > 4.0e6
    assert growth < bound
    grad = sd.grad.clone()
    sd.grad = None
    loss_general, n_general = M.pairwise_loss(sd, yd, gd, pairloss_func=lambda p, n, w: M.hinge_loss_func(p, n, w, margin=margin),
                                              return_num_pair=True, label_pair_to_weight_func=table)
    loss_general.backward()
    gerr = (grad - sd.grad).abs().max().item()
    print('fused route %.9g  general route %.9g  grad err %.3g of max %.3g' % (loss.item(), loss_general.item(), gerr, sd.grad.abs().max().item()))
    assert n_general.item() == n_pair.item()
    assert abs(loss.item() - loss_general.item()) <= RTOL * max(1.0, abs(loss_general.item()))
    assert gerr <= RTOL * sd.grad.abs().max().item()


def test_lambda_takes_the_general_route(dev, monkeypatch):
    M = _mod()
    g, s, y, mask = _batch('b1000')
    table, wf = _rule(M, 'explicit')
    margin = 0.5 + KINK
    _assert_off_the_kink(g, s, margin, 2.0)
    calls = []
    real = M.pair_indices

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(M, 'pair_indices', spy)
    lf = lambda p, n, w: M.hinge_loss_func(p, n, w, margin=margin, factor=2.0)              # noqa: E731  (not the function itself: the general route)
    got = _run(M, dev, g, s, y, mask, -0.5, False, pairloss_func=lf, label_pair_to_weight_func=table)
    assert calls
    _check(got, _oracle(('b1000', 'f32'), g, s, y, mask, 'hinge', margin, 2.0, wf, -0.5, False))


# ---- the C entry itself --------------------------------------------------------------------------------------------------------------------
def _abi_call(dev, g, s, y, mask, table, kind, packed, flags_extra=0, margin=0.5, factor=1.0, power=-0.5, n_values=None, B=None):
    """recnow_pair_kind_fwdbwd behind the matching count call; returns (return code, loss, dscores).  packed: hand the count's workspace over
    with RECNOW_PAIR_MEMBERS_PACKED, else a fresh workspace that the entry has to pack itself."""
    from rec_now_amd import _lib
    M = _mod()
    lib = _lib.load()
    seg = M.group_rows(_t(g).to(dev))
    nB = seg.B if B is None else B
    sd, yd = _t(s).to(dev), _t(y).to(dev)
    md = None if mask is None else _t(mask).to(dev).to(torch.uint8)
    cnt_row = torch.empty(seg.B, dtype=torch.int32, device=dev)
    cnt_super = torch.empty(seg.B, dtype=torch.int64, device=dev)
    n_pair = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _lib.workspace(lib.recnow_pairwise_workspace_bytes(seg.B), dev)
    P, st = _lib.ptr, _lib.stream()
    if table is not None:
        vals, w = table.on_device(dev)
        K, flags = table.n_values, 0
        _lib.call('recnow_pair_table_count', P(sd), P(yd), P(md), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), seg.B, flags,
                  P(vals), K, P(w), P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
    else:
        vals, w, K, flags = None, None, 0, 1                   # RECNOW_PAIR_LABEL_GT
        _lib.call('recnow_pair_count', P(sd), P(yd), P(md), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), seg.B, flags,
                  P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
    if not packed:
        ws = torch.full_like(ws, 0xFF)                         # nothing of the count call's members survives
    loss = torch.full((), 7.0, dtype=torch.float32, device=dev)
    dscores = torch.zeros(seg.B, dtype=torch.float32, device=dev)
    rc = lib.recnow_pair_kind_fwdbwd(P(sd), P(yd), P(md), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), P(cnt_super), P(n_pair),
                                     nB, (flags | (256 if packed else 0)) ^ flags_extra, kind, margin, P(vals), K if n_values is None else n_values,
                                     P(w), factor, power, 1, P(loss), P(dscores), P(ws), ws.numel(), st)
    torch.cuda.synchronize()
    return rc, loss.item(), dscores.cpu().numpy()


@pytest.mark.parametrize('rule', ['default', 'sym'])
def test_c_entry_packs_the_members_itself(dev, rule):
    """Without RECNOW_PAIR_MEMBERS_PACKED the entry packs the rows (class ids and the unknown-label flag with a table): the same bits as on the
    count call's workspace, on b2900 (LDS stage, wave per row, global-memory walk)."""
    M = _mod()
    g, s, y, mask = _batch('b2900')
    table, _ = _rule(M, rule)
    for kind in (1, 2, 3):
        a = _abi_call(dev, g, s, y, mask, table, kind, packed=True)
        b = _abi_call(dev, g, s, y, mask, table, kind, packed=False)
        assert a[0] == 0 and b[0] == 0
        assert np.isfinite(a[1]) and np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes()
        assert a[2].tobytes() == b[2].tobytes() and np.abs(a[2]).max() > 0
    if rule == 'sym':                                          # the flag is raised by the entry's own packing as well
        y2 = y.copy()
        y2[int(np.flatnonzero(mask)[3])] = 9.0
        rc, loss, grad = _abi_call(dev, g, s, y2, mask, table, 1, packed=False)
        assert rc == 0 and np.isnan(loss) and np.isnan(grad).all()


def test_c_entry_refuses_bad_arguments(dev):
    M = _mod()
    g, s, y, mask = _batch('b64')
    table, _ = _rule(M, 'sym')
    EINVAL = -1                                                # RECNOW_EINVAL of include/recnow.h
    inf, nan = float('inf'), float('nan')
    for t in (table, None):
        assert _abi_call(dev, g, s, y, mask, t, 1, True)[0] == 0
        for kind in (0, 4, -1):
            assert _abi_call(dev, g, s, y, mask, t, kind, True)[0] == EINVAL
        for bad in (inf, -inf, nan):
            assert _abi_call(dev, g, s, y, mask, t, 1, True, margin=bad)[0] == EINVAL
            assert _abi_call(dev, g, s, y, mask, t, 3, True, factor=bad)[0] == EINVAL
        for extra in (4, 8, 512):                              # flags that are not listed
            assert _abi_call(dev, g, s, y, mask, t, 2, True, flags_extra=extra)[0] == EINVAL
    assert _abi_call(dev, g, s, y, mask, None, 1, True, flags_extra=1)[0] == EINVAL        # no table and no RECNOW_PAIR_LABEL_GT
    assert _abi_call(dev, g, s, y, mask, table, 1, True, flags_extra=1)[0] == EINVAL       # RECNOW_PAIR_LABEL_GT beside a table
    for nv in (0, 17, -3):
        assert _abi_call(dev, g, s, y, mask, table, 1, True, n_values=nv)[0] == EINVAL
    rc, loss, grad = _abi_call(dev, g, s, y, mask, table, 1, True, B=0)                    # B == 0 writes loss = 0
    assert rc == 0 and loss == 0.0

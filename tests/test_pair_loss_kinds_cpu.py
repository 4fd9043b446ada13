"""CPU: hinge_loss_func, squared_hinge_loss_func and margin_bpr_loss_func of rec_now_amd.rec_block.pairwise_loss_from_batch -- the option
parser that decides whether `pairwise_loss` stays on the fused route, and the vector forms (plain torch ops on the tensors' own device)
against closed-form fp64 restatements written here."""
import functools

import numpy as np
import pytest
import torch


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


NAMES = {'hinge_loss_func': 'hinge', 'squared_hinge_loss_func': 'squared_hinge', 'margin_bpr_loss_func': 'margin_bpr'}


def _closed_form(kind, p, n, w, margin, factor, reduce_mean):
    """fp64 numpy, element by element from the definition."""
    u = margin - factor * (p.astype(np.float64) - n.astype(np.float64))
    if kind == 'hinge':
        f = np.maximum(u, 0.0)
    elif kind == 'squared_hinge':
        f = np.maximum(u, 0.0) ** 2
    else:
        f = np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))
    s = float((f * (1.0 if w is None else w.astype(np.float64))).sum())
    return s / (u.size + 1e-10) if reduce_mean else s


# ---- the option parser ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fname', sorted(NAMES))
def test_parser_recognises_the_functions_and_keyword_partials(fname):
    M = _mod()
    F = getattr(M, fname)
    k = NAMES[fname]
    assert M._kind_options(F) == (k, 1.0, 1.0, True)
    assert M._kind_options(functools.partial(F)) == (k, 1.0, 1.0, True)
    assert M._kind_options(functools.partial(F, margin=0.25)) == (k, 0.25, 1.0, True)
    assert M._kind_options(functools.partial(F, factor=2, reduce_mean=False)) == (k, 1.0, 2.0, False)
    assert M._kind_options(functools.partial(F, margin=0, factor=0.5, reduce_mean=True)) == (k, 0.0, 0.5, True)


@pytest.mark.parametrize('fname', sorted(NAMES))
def test_parser_rejects_what_the_kernels_cannot_compute(fname):
    M = _mod()
    F = getattr(M, fname)
    assert M._kind_options(functools.partial(F, 1.0)) is None                        # a positional argument
    assert M._kind_options(functools.partial(F, weights=None)) is None               # a foreign keyword
    assert M._kind_options(functools.partial(F, margin=1.0, scale=2.0)) is None
    assert M._kind_options(lambda p, n, w: F(p, n, w)) is None                       # a lambda is just another callable
    assert M._kind_options(M.bpr_loss_func) is None
    assert M._kind_options(functools.partial(M.bpr_loss_func, factor=0.7)) is None
    assert M._bpr_options(F) is None and M._bpr_options(functools.partial(F, factor=0.7)) is None
    for bad in (float('inf'), float('-inf'), float('nan'), '1.0', None, torch.tensor(1.0), True):
        with pytest.raises(ValueError, match='margin'):
            M._kind_options(functools.partial(F, margin=bad))
    for bad in (float('inf'), float('nan'), 'x'):
        with pytest.raises(ValueError, match='factor'):
            M._kind_options(functools.partial(F, factor=bad))


def test_fused_entry_refuses_bad_kind_and_margin():
    M = _mod()
    z = torch.zeros(4)
    with pytest.raises(ValueError, match='kind'):
        M.pairwise_loss_fused(z, z, z, kind='exp')
    with pytest.raises(ValueError, match='margin'):
        M.pairwise_loss_fused(z, z, z, kind='hinge', margin=float('nan'))
    with pytest.raises(ValueError, match='margin'):
        M.pairwise_loss_fused(z, z, z, margin=1.0)                                   # the BPR term has no margin
    with pytest.raises(TypeError):
        M.pairwise_loss_fused(z, z, z, kind='hinge', label_pair_weights=lambda a, b: a - b)
    with pytest.raises(TypeError):
        M.pairwise_loss_fused(z, z, z, None, 0.0, None, 1.0, True, None, True, None, 'hinge')    # kind is keyword only


# ---- the vector forms -------------------------------------------------------------------------------------------------------------------
def _vectors(P=1537, seed=11):
    rng = np.random.default_rng(seed)
    return rng.normal(size=P).astype(np.float32) * 2, rng.normal(size=P).astype(np.float32) * 2, (rng.random(P) * 3).astype(np.float32)


@pytest.mark.parametrize('fname', sorted(NAMES))
@pytest.mark.parametrize('margin,factor,reduce_mean,weighted', [(1.0, 1.0, True, False), (0.3, 0.7, True, True), (2.0, 2.0, False, True),
                                                                (0.0, 1.0, False, False), (-0.5, 0.5, True, True)])
def test_vector_form_equals_the_closed_form(fname, margin, factor, reduce_mean, weighted):
    M = _mod()
    p, n, w = _vectors()
    if not weighted:
        w = None
    want = _closed_form(NAMES[fname], p, n, w, margin, factor, reduce_mean)
    F = getattr(M, fname)
    # fp64 tensors: the closed form to rounding of the sum
    got64 = F(torch.from_numpy(p).double(), torch.from_numpy(n).double(), None if w is None else torch.from_numpy(w).double(), margin, factor,
              reduce_mean)
    assert got64.dtype == torch.float64
    assert abs(got64.item() - want) <= 1e-12 * max(1.0, abs(want))
    # fp32 tensors: P terms of relative rounding 2**-24 each, summed pairwise by torch
    got32 = F(torch.from_numpy(p), torch.from_numpy(n), None if w is None else torch.from_numpy(w), margin=margin, factor=factor,
              reduce_mean=reduce_mean)
    assert got32.dtype == torch.float32
    assert abs(got32.item() - want) <= 2e-6 * max(1.0, abs(want))
    # default arguments: margin 1, factor 1, mean
    if (margin, factor, reduce_mean, weighted) == (1.0, 1.0, True, False):
        assert F(torch.from_numpy(p), torch.from_numpy(n)).item() == got32.item()


def test_hinge_is_margin_ranking_loss():
    M = _mod()
    p, n, _ = _vectors()
    pt, nt = torch.from_numpy(p), torch.from_numpy(n)
    want = torch.nn.functional.margin_ranking_loss(pt, nt, torch.ones_like(pt), margin=1.0)
    got = M.hinge_loss_func(pt, nt)
    # the same fp32 terms; the two sums may be taken in another order (a few of 2**-24 relative), the 1e-10 of the mean is below fp32 rounding
    assert abs(got.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item()))


@pytest.mark.parametrize('fname', sorted(NAMES))
def test_reduce_mean_false_is_the_raw_sum_and_the_mean_counts_every_pair(fname):
    M = _mod()
    F = getattr(M, fname)
    p, n, w = (torch.from_numpy(a).double() for a in _vectors(P=400))
    raw = F(p, n, w, reduce_mean=False)
    mean = F(p, n, w)
    # P = 400 counts the pairs whose hinge term is 0, too
    assert abs(mean.item() - raw.item() / (400 + 1e-10)) <= 1e-12 * max(1.0, abs(mean.item()))
    assert abs(F(p, n, None, 0.5, 1.0, False).item() - _closed_form(NAMES[fname], p.numpy(), n.numpy(), None, 0.5, 1.0, False)) < 1e-9


@pytest.mark.parametrize('fname', sorted(NAMES))
def test_weights_are_constants(fname):
    M = _mod()
    F = getattr(M, fname)
    p, n, w = (torch.from_numpy(a).double() for a in _vectors(P=300))
    p.requires_grad_(True)
    n.requires_grad_(True)
    w.requires_grad_(True)
    F(p, n, w * 1.0, margin=0.5).backward()
    assert w.grad is None
    assert p.grad is not None and torch.equal(p.grad, -n.grad)
    assert float(p.grad.abs().max()) > 0.0


def test_gradients_equal_the_closed_form_derivatives():
    M = _mod()
    pn, nn_, wn = _vectors(P=500)
    margin, factor = 0.75, 0.5
    u = margin - factor * (pn.astype(np.float64) - nn_.astype(np.float64))
    want = {'hinge_loss_func': (u > 0) * 1.0, 'squared_hinge_loss_func': 2 * np.maximum(u, 0), 'margin_bpr_loss_func': 1 / (1 + np.exp(-u))}
    for fname, df in want.items():
        p = torch.from_numpy(pn).double().requires_grad_(True)
        getattr(M, fname)(p, torch.from_numpy(nn_).double(), torch.from_numpy(wn).double(), margin, factor, reduce_mean=False).backward()
        assert np.allclose(p.grad.numpy(), -factor * wn.astype(np.float64) * df, rtol=1e-12, atol=1e-14)


def test_kink_subgradient_is_zero():
    M = _mod()
    # u = 1 - (pos - neg) is exactly 0 for the first pair, positive for the second, negative for the third
    for F in (M.hinge_loss_func, M.squared_hinge_loss_func):
        p = torch.tensor([2.0, 0.5, 4.0], requires_grad=True)
        n = torch.tensor([1.0, 0.0, 1.0], requires_grad=True)
        loss = F(p, n, reduce_mean=False)
        loss.backward()
        assert p.grad[0].item() == 0.0 and n.grad[0].item() == 0.0
        assert p.grad[1].item() < 0.0 and n.grad[1].item() > 0.0
        assert p.grad[2].item() == 0.0 and n.grad[2].item() == 0.0
    p = torch.tensor([2.0], requires_grad=True)
    M.margin_bpr_loss_func(p, torch.tensor([1.0]), reduce_mean=False).backward()
    assert p.grad[0].item() == -0.5                                                    # sigma(0): the smooth kind has no kink


@pytest.mark.parametrize('fname', sorted(NAMES))
def test_non_finite_options_are_refused_by_the_functions(fname):
    M = _mod()
    F = getattr(M, fname)
    z = torch.zeros(3)
    for kw in ({'margin': float('inf')}, {'margin': float('nan')}, {'factor': float('inf')}, {'margin': 'a'}, {'factor': None},
               {'margin': torch.tensor(1.0)}):
        with pytest.raises(ValueError):
            F(z, z, **kw)


def test_abi_names_match_the_python_constants():
    import os
    import re
    M = _mod()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'recnow.h')).read()
    got = dict(re.findall(r'#define RECNOW_PAIR_KIND_([A-Z_]+) (\d+)', text))
    assert got == {'HINGE': str(M._KIND_HINGE), 'SQUARED_HINGE': str(M._KIND_SQUARED_HINGE), 'MARGIN_LOGISTIC': str(M._KIND_MARGIN_LOGISTIC)}

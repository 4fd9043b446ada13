"""GPU tests of the head-Q form of the fused scoring head (csrc/dcnmix.hip `mix_head_q`): in split precision on the launch-per-product
route the forward takes the score as the row dot T2g_{L-1} . Q with Q = x Wh^T (no output product of the top layer, no O_{L-1}), the backward reads Q
as the head's dT2g and forms the head's part of d loss / d x as the second K = 144 half of layer 0's one-go product (c2_mode 7 / 8 of the short-K
kernel, csrc/gemm_shortk.hip).

  1. every piece of the new form against the fp64 oracle (oracle/dense_ref.py through tests/_chunked_oracle.py + the C pair oracle) at the suite's 1e-5
     bound: loss, pair count, scores, d loss / d x, every weight gradient; L = 2 reaches c2_mode 8, L = 3 c2_mode 7; B = 768 is three 256-row groups,
     D = 1024 puts eight column tiles behind one row tile; with and without d loss / d x;
  2. the route ran: one RN_TAG_GEMM_SHORTK launch fewer per step than in exact fp32, and scores that are not those of the exact-fp32 forward;
  3. the backward follows the MIX_HEAD_Q stamp of `saved`, not the rule of the moment: precision flipped to exact fp32 (O_{L-1} recomputed), the row-block
     backward refused on a head-Q `saved`, and the unchanged path behind a row-block forward;
  4. zero rows of x score the head bias bit for bit.
Inputs are scaled so that the scores are of O(0.3), as bench.py's parity step does.
Reference: /root/reference/rec_now/layers/dcn_mix_layer.py:114-151, multi_dense_layer.py:80-94, rec_block/pairwise_loss_from_batch.py:228-279."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _chunked_oracle import gemm_precision
from test_step_gpu import _model, _oracle_step

pytestmark = pytest.mark.gpu

S, N = 64, 2
HEAD_GAIN = 4.0             # test_step_gpu._model's 40 spreads the scores over +-10; 4 -> |score| of O(0.3) (checked against the oracle in _case)
RN_TAG_GEMM_SHORTK = 5      # csrc/prof.hpp
BOUND = 1e-5


class _env:
    """Route switches that the library reads per call: set for the block, restored behind it."""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


_CASES = {}


def _case(dev, B, D, L):
    """Model, inputs and the fp64 oracle of one shape: computed once, shared by the tests, never changed."""
    key = (B, D, L)
    if key not in _CASES:
        x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 5000 + B + D + L, head_gain=HEAD_GAIN)
        rs, rloss, rds, rP, rdx, rgrads, named = _oracle_step(x, groups, labels, cross, head, L, grouped=False)
        assert rP > 0 and abs(rloss - np.log(2.0)) > 1e-3 and 0.1 < np.median(np.abs(rs)) < 1.0, (rP, rloss, np.median(np.abs(rs)))
        _CASES[key] = dict(x=x, groups=groups, labels=labels, xd=xd, yd=yd, gd=gd, cross=cross, head=head, rs=rs, rloss=rloss, rds=rds, rP=rP, rdx=rdx,
                           rgrads=rgrads, named=named)
    return _CASES[key]


def _rel(a, b, scale=None):
    a = a.detach().cpu().double().numpy() if hasattr(a, 'detach') else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max() if scale is None else scale, 1e-30))


def _check(c, step, what, need_dx=True):
    """loss, pair count, scores, d loss / d x and every weight gradient against the oracle; the worst tensor is reported."""
    assert int(step.n_pair.item()) == c['rP'], what
    errs = {'loss': _rel(step.loss, np.float64(c['rloss'])), 'scores': _rel(step.scores, c['rs'])}
    if need_dx:
        errs['dx'] = _rel(step.dx, c['rdx'])
    for name, p in c['named'].items():
        # d loss / d head bias = sum of dscores cancels to ~0: on the scale of its terms (as tests/test_step_gpu.py)
        errs[name] = _rel(p.grad, c['rgrads'][name], scale=np.abs(c['rds']).sum() if name == 'head/bias' else None)
    worst = max(errs, key=errs.get)
    print('%s: worst %s %.3g of %d tensors' % (what, worst, errs[worst], len(errs)))
    assert np.isfinite(list(errs.values())).all() and errs[worst] <= BOUND, (what, worst, errs[worst])


def _fresh(step):
    for g in step.grads:
        g.fill_(float('nan'))
    if step.dx is not None:
        step.dx.fill_(float('nan'))
    step.scores.fill_(float('nan'))
    step._bind_grads()


def _step(c, need_dx=True):
    from rec_now_amd.step import DCNMixPairwiseStep
    return DCNMixPairwiseStep(c['cross'], c['head'], c['xd'], c['yd'], c['gd'], need_dx=need_dx)


@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('B', [512, 768])
@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('D', [256, 1024])
def test_head_q_step_vs_oracle(dev, D, L, B, need_dx):
    c = _case(dev, B, D, L)
    step = _step(c, need_dx)
    _fresh(step)
    with _env(RECNOW_TILE='0'), gemm_precision('bf16x3'):
        assert step.route_code() == 0
        step.run()
        torch.cuda.synchronize()
    _check(c, step, 'head-Q D=%d L=%d B=%d dx=%d' % (D, L, B, need_dx), need_dx)


def _shortk_launches(step):
    from rec_now_amd import _lib
    lib = _lib.load()
    cap = 1024
    _lib.check(lib.recnow_prof_enable(cap), 'recnow_prof_enable')
    try:
        _lib.check(lib.recnow_prof_sample_every(1), 'recnow_prof_sample_every')
        step.run()
        torch.cuda.synchronize()
        t, t0, t1 = (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
        n = lib.recnow_prof_intervals(t, t0, t1, cap)
        assert 0 < n < cap and lib.recnow_prof_dropped() == 0, n
        return sum(1 for i in range(n) if t[i] == RN_TAG_GEMM_SHORTK)
    finally:
        lib.recnow_prof_enable(0)


@pytest.mark.parametrize('L', [2, 3])
def test_head_q_route_ran(dev, L):
    """Per step the exact-fp32 product route runs the L products that leave a layer and the L input-gradient products on the short-K kernel; head-Q
    drops the top layer's output product (its dT2g product, now in the forward, is a long-K launch in both)."""
    c = _case(dev, 512, 256, L)
    step = _step(c)
    with _env(RECNOW_TILE='0'):
        with gemm_precision('f32'):
            n_exact = _shortk_launches(step)
            scores_exact = step.scores.clone()
        with gemm_precision('bf16x3'):
            n_q = _shortk_launches(step)
            scores_q = step.scores.clone()
    assert n_exact == 2 * L and n_q == n_exact - 1, (n_exact, n_q)
    assert not torch.equal(scores_q, scores_exact)


@pytest.mark.parametrize('L', [2, 3])
def test_backward_in_exact_fp32_behind_a_head_q_forward(dev, L):
    """The fallback: the stamp says head-Q, this backward cannot run the K = 288 form -> O_{L-1} is recomputed, Q is the head's dT2g."""
    from rec_now_amd.step import _BACKWARD, _FORWARD, _GROUP, _LOSS
    c = _case(dev, 512, 256, L)
    step = _step(c)
    _fresh(step)
    with _env(RECNOW_TILE='0'):
        with gemm_precision('bf16x3'):
            step._call(_GROUP | _FORWARD | _LOSS)
        with gemm_precision('f32'):
            step._call(_BACKWARD, L - 1, 0)
        torch.cuda.synchronize()
    _check(c, step, 'head-Q forward, exact-fp32 backward, L=%d' % L)


def test_row_block_backward_is_refused_on_a_head_q_saved(dev):
    """RECNOW_TILE=1 and exact fp32 by the time of the backward: the rule of the moment says row-block chain, which reads an O_{L-1} that a head-Q
    forward never wrote (the buffers start as NaN here).  The stamp decides: product route."""
    from rec_now_amd.step import _BACKWARD, _FORWARD, _GROUP, _LOSS
    c = _case(dev, 512, 256, 2)
    step = _step(c)
    step.ws.view(torch.uint8).fill_(0xff)
    _fresh(step)
    with _env(RECNOW_TILE='0'), gemm_precision('bf16x3'):
        step._call(_GROUP | _FORWARD | _LOSS)
    with _env(RECNOW_TILE='1'), gemm_precision('f32'):
        assert step.route_code() == 1
        step._call(_BACKWARD, 1, 0)
    torch.cuda.synchronize()
    _check(c, step, 'head-Q forward, RECNOW_TILE=1 exact-fp32 backward')


def test_product_backward_behind_a_row_block_forward_is_unchanged(dev):
    """Row-block forward (RECNOW_TILE=1, exact fp32: not head-Q, O_{L-1} written) with the product-route backward (RECNOW_TILE_BWD=0)."""
    c = _case(dev, 512, 256, 2)
    step = _step(c)
    _fresh(step)
    with _env(RECNOW_TILE='1', RECNOW_TILE_BWD='0'), gemm_precision('f32'):
        assert step.route_code() == 1
        step.run()
        torch.cuda.synchronize()
    _check(c, step, 'row-block forward, product-route backward')


def test_zero_rows_score_the_head_bias(dev):
    c = _case(dev, 512, 256, 2)
    from rec_now_amd.step import DCNMixPairwiseStep
    xz = c['xd'].clone()
    xz[-256:] = 0.0
    step = DCNMixPairwiseStep(c['cross'], c['head'], xz, c['yd'], c['gd'])
    step.scores.fill_(float('nan'))
    with _env(RECNOW_TILE='0'), gemm_precision('bf16x3'):
        step.run()
        torch.cuda.synchronize()
    bias = c['head'].bias.detach().reshape(-1)[0]
    assert torch.equal(step.scores[-256:], bias.expand(256)) and not torch.equal(step.scores[:256], bias.expand(256))

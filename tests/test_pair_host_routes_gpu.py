"""Which library entries the host side of the in-batch pairwise loss calls, and in which order, route by route.

`rec_now_amd._lib.call` is wrapped with a recorder; every case runs forward and backward on one batch of 64 rows in 5 float32 groups with four
label levels and a mask with a few zeros, and the recorded entry names -- the grouping entries included -- must equal the case's row of CASES
exactly.  The table was written from the host code, entry by entry; it is what "the same route" means on the host side, where the numeric
tests see only the result.  The lambda cases also pin the workspace the counting entry is handed: the larger one of the NDCG walk."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 64
KEYS, SEGMENTS = 'recnow_group_keys', 'recnow_group_segments'
COUNT, TABLE_COUNT = 'recnow_pair_count', 'recnow_pair_table_count'
LEVELS = [0.0, 1.0, 2.0, 3.0]


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _batch(dev):
    i = np.arange(B)
    rng = np.random.default_rng(11)
    g = torch.from_numpy((i % 5).astype(np.float32)).to(dev)
    g2 = torch.from_numpy((i // 2 % 3).astype(np.float32)).to(dev)
    y = torch.from_numpy((i * 7 % 4).astype(np.float32)).to(dev)
    mask = torch.from_numpy(i % 13 != 5).to(dev)
    s = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(dev)
    return g, g2, y, mask, s


def _table(M):
    return M.LabelPairWeightTable(LEVELS, lambda a, b: (a - b).abs() + 0.5)


def _lam():
    from rec_now_amd.rec_block.ndcg import NDCGLambdaWeight
    return NDCGLambdaWeight()


# name -> (call, expected entries).  call(M, s, y, g, g2, mask, seg) -> loss; seg = group_rows(g), built before the recorder is on
CASES = {
    'default-one-tensor': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, mask=mask),
        ['recnow_pairwise_loss']),
    'default-two-tensors-power0': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, [g, g2], mask=mask),
        [KEYS, KEYS, SEGMENTS, 'recnow_pair_bpr_onepass', 'recnow_pair_scale_grad']),
    'power-float32-small': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, mask=mask, click_occurance_power=-0.5),
        ['recnow_group_pack_small', COUNT, 'recnow_pair_bpr_fwdbwd']),
    'power-int64-segments': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g.to(torch.int64), mask=mask, click_occurance_power=-0.5),
        [KEYS, SEGMENTS, COUNT, 'recnow_pair_bpr_fwdbwd']),
    'fused-with-segments-power0': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss_fused(s, y, None, mask=mask, segments=seg)[0],
        ['recnow_pair_bpr_onepass', 'recnow_pair_scale_grad']),
    'table-bpr': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, mask=mask, label_pair_to_weight_func=_table(M)),
        [KEYS, SEGMENTS, TABLE_COUNT, 'recnow_pair_table_bpr_fwdbwd']),
    'kind-with-table': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, pairloss_func=M.hinge_loss_func, mask=mask,
                                                          label_pair_to_weight_func=_table(M)),
        [KEYS, SEGMENTS, TABLE_COUNT, 'recnow_pair_kind_fwdbwd']),
    'kind-without-table': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, pairloss_func=functools.partial(M.margin_bpr_loss_func, margin=0.3),
                                                          mask=mask),
        [KEYS, SEGMENTS, COUNT, 'recnow_pair_kind_fwdbwd']),
    'lambda-with-table': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, mask=mask, label_pair_to_weight_func=_table(M), lambda_weight=_lam()),
        [KEYS, SEGMENTS, TABLE_COUNT, 'recnow_pair_lambda_terms', 'recnow_pair_lambda_fwdbwd']),
    'lambda-without-table': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, pairloss_func=M.squared_hinge_loss_func, mask=mask, lambda_weight=_lam()),
        [KEYS, SEGMENTS, COUNT, 'recnow_pair_lambda_terms', 'recnow_pair_lambda_fwdbwd']),
    'general-wrapped-pairloss': (
        lambda M, s, y, g, g2, mask, seg: M.pairwise_loss(s, y, g, pairloss_func=lambda p, n, w: M.bpr_loss_func(p, n, w), mask=mask),
        [KEYS, SEGMENTS, COUNT, 'recnow_pair_offsets', 'recnow_pair_emit', 'recnow_bpr_loss_fwdbwd']),
}


def _record(monkeypatch, dev, name, one_call=True):
    from rec_now_amd import _lib
    M = _mod()
    g, g2, y, mask, s = _batch(dev)
    seg = M.group_rows(g)                              # before the recorder: a caller's own, earlier, work
    monkeypatch.setattr(M, '_ONE_CALL', one_call)
    calls = []
    real = _lib.call

    def recorder(entry, *args):
        calls.append((entry, args))
        return real(entry, *args)

    monkeypatch.setattr(_lib, 'call', recorder)
    s = s.clone().requires_grad_(True)
    loss = CASES[name][0](M, s, y, g, g2, mask, seg)
    loss.backward()
    torch.cuda.synchronize()
    assert s.grad is not None and bool(torch.isfinite(s.grad).all()) and bool(torch.isfinite(loss))
    assert float(s.grad.abs().max()) > 0
    return calls


@pytest.mark.parametrize('name', list(CASES))
def test_entries_called_in_order(dev, monkeypatch, name):
    calls = _record(monkeypatch, dev, name)
    got = [c[0] for c in calls]
    print('HOST ROUTE %s: %s' % (name, ' -> '.join(got)))
    assert got == CASES[name][1]


def test_small_route_power0_without_the_one_call_switch(dev, monkeypatch):
    """RECNOW_PAIR_ONE_CALL=0 (here: the module flag it sets): one float32 tensor at power 0 takes pack-small and the one-walk entry."""
    calls = _record(monkeypatch, dev, 'default-one-tensor', one_call=False)
    got = [c[0] for c in calls]
    print('HOST ROUTE default-one-tensor, piecewise: %s' % ' -> '.join(got))
    assert got == ['recnow_group_pack_small', 'recnow_pair_bpr_onepass', 'recnow_pair_scale_grad']


@pytest.mark.parametrize('name', ['lambda-with-table', 'lambda-without-table'])
def test_lambda_count_runs_on_the_lambda_workspace(dev, monkeypatch, name):
    """Every entry of the lambda route is handed the one workspace of recnow_pair_lambda_workspace_bytes, the counting entry included; the
    other families count on recnow_pairwise_workspace_bytes."""
    from rec_now_amd import _lib
    lib = _lib.load()
    want = max(int(lib.recnow_pair_lambda_workspace_bytes(B)), 16)
    plain = max(int(lib.recnow_pairwise_workspace_bytes(B)), 16)
    calls = _record(monkeypatch, dev, name)
    sizes = {entry: args[-2] for entry, args in calls if entry.startswith('recnow_pair_')}
    print('HOST ROUTE %s workspaces: %s (lambda %d, plain %d)' % (name, sizes, want, plain))
    assert len(sizes) == 3 and all(n == want for n in sizes.values())
    other = 'kind-with-table' if name == 'lambda-with-table' else 'kind-without-table'
    sizes = {entry: args[-2] for entry, args in _record(monkeypatch, dev, other) if entry.startswith('recnow_pair_')}
    assert len(sizes) == 2 and all(n == plain for n in sizes.values())

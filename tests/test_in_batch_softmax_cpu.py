"""CPU: the fp64 oracle of the in-batch sampled softmax (tests/_in_batch_softmax_oracle.py) pinned to a hand-worked example and to torch fp64
autograd of the cross-entropy restatement, its defining properties, and everything of rec_now_amd.rec_block.in_batch_softmax that needs no GPU:
argument errors, the D > 128 refusal, the CPU refusal, the B = 0 path, and the host-only entry points of the library."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _in_batch_softmax_oracle as O
from rec_now_amd import _lib
from rec_now_amd.rec_block import in_batch_softmax as M


def _oracle(c, **over):
    kw = dict(item_ids=c['item_ids'], log_q=c['log_q'], temperature=c['temperature'], mask=c['mask'])
    kw.update(over)
    q, v = kw.pop('query', c['query']), kw.pop('item', c['item'])
    return O.in_batch_softmax_oracle(q, v, **kw)


def test_a_hand_worked_example():
    """B = 3, D = 2, tau = 1: logits [[1, 0, 0], [0, 1, 0], [1, 1, 0]]."""
    q = np.array([[1., 0.], [0., 1.], [1., 1.]])
    v = np.array([[1., 0.], [0., 1.], [0., 0.]])
    r = O.in_batch_softmax_oracle(q, v)
    e = math.e
    l0, l2 = math.log(e + 2) - 1, math.log(2 * e + 1)
    assert np.allclose(r['row_loss'], [l0, l0, l2], rtol=1e-14, atol=0) and r['n'] == 3
    assert abs(r['loss'] - (2 * l0 + l2) / 3) <= 1e-15
    p00, p01, p02, p22 = e / (e + 2), 1 / (e + 2), 1 / (e + 2), 1 / (2 * e + 1)
    assert np.allclose(r['dq'][0], [(p00 - 1) / 3, p01 / 3], rtol=1e-14, atol=0)
    assert np.allclose(r['dv'][2], [(p02 + (p22 - 1)) / 3, (p02 + (p22 - 1)) / 3], rtol=1e-14, atol=0)
    # with log_q = log [1/2, 1/4, 1/4] row 0 sees [1 + ln 2, ln 4, ln 4]
    r = O.in_batch_softmax_oracle(q, v, log_q=np.log([0.5, 0.25, 0.25]))
    assert abs(r['row_loss'][0] - (math.log(2 * e + 8) - 1 - math.log(2))) <= 1e-15
    # ids [5, 5, 6]: rows 0 and 1 lose each other
    r = O.in_batch_softmax_oracle(q, v, item_ids=[5, 5, 6])
    assert abs(r['row_loss'][0] - (math.log(e + 1) - 1)) <= 1e-15 and r['p'][0, 1] == 0 and r['p'][1, 0] == 0
    assert np.allclose(O.in_batch_softmax_oracle(q, v, item_ids=[5, 5, 6], remove_accidental_hits=False)['row_loss'], [l0, l0, l2], rtol=1e-14)


@pytest.mark.parametrize('config', O.CONFIGS)
@pytest.mark.parametrize('B,D', [(1, 3), (7, 5), (41, 16)])
def test_the_oracle_is_torch_fp64_autograd_of_the_cross_entropy(B, D, config):
    c = O.make_case(B, D, config, 16)
    r = _oracle(c)
    q = torch.from_numpy(c['query']).double().requires_grad_(True)
    v = torch.from_numpy(c['item']).double().requires_grad_(True)
    on = np.ones(B, dtype=bool) if c['mask'] is None else c['mask']
    logits = q @ v.T / c['temperature']
    if c['log_q'] is not None:
        logits = logits - torch.from_numpy(c['log_q']).double()[None, :]
    drop = torch.from_numpy(np.broadcast_to(~on[None, :], (B, B)).copy())
    if c['item_ids'] is not None:
        ids = torch.from_numpy(c['item_ids'])
        drop = drop | (ids[None, :] == ids[:, None])
    logits = logits.masked_fill(drop & ~torch.eye(B, dtype=torch.bool), float('-inf'))
    rows = torch.from_numpy(np.flatnonzero(on))
    if rows.numel() == 0:
        assert r['loss'] == 0.0 and r['n'] == 0 and not r['dq'].any() and not r['dv'].any()
        return
    loss = F.cross_entropy(logits[rows], rows)
    gq, gv = torch.autograd.grad(loss, [q, v])
    assert abs(r['loss'] - loss.item()) <= 1e-12 and r['n'] == on.sum()
    assert np.abs(r['dq'] - gq.numpy()).max() <= 1e-12 and np.abs(r['dv'] - gv.numpy()).max() <= 1e-12
    comp = O.composition(q, v, None if c['item_ids'] is None else torch.from_numpy(c['item_ids']),
                         None if c['log_q'] is None else torch.from_numpy(c['log_q']), c['temperature'],
                         None if c['mask'] is None else torch.from_numpy(c['mask']))
    assert abs(comp[0].item() - r['loss']) <= 1e-12
    assert np.abs(comp[1].detach().numpy()[on] - r['lse'][on]).max() <= 1e-12 and np.abs(comp[2].detach().numpy()[on] - r['pos'][on]).max() <= 1e-12


def test_a_constant_added_to_log_q_changes_nothing():
    c = O.make_case(23, 6, 'all', 8)
    a, b = _oracle(c), _oracle(c, log_q=c['log_q'].astype(np.float64) + 3.25)
    assert abs(a['loss'] - b['loss']) <= 1e-12 and np.abs(a['dq'] - b['dq']).max() <= 1e-13 and np.abs(a['dv'] - b['dv']).max() <= 1e-13


def test_all_distinct_ids_equal_no_ids():
    c = O.make_case(19, 4, 'log_q', 8)
    a, b = _oracle(c), _oracle(c, item_ids=np.arange(19)[::-1] * 3)
    assert a['loss'] == b['loss'] and np.array_equal(a['dq'], b['dq']) and np.array_equal(a['dv'], b['dv'])


def test_a_mask_equals_deleting_the_rows():
    c = O.make_case(29, 5, 'all', 8)
    keep = np.flatnonzero(c['mask'])
    a = _oracle(c)
    b = O.in_batch_softmax_oracle(c['query'][keep], c['item'][keep], c['item_ids'][keep], c['log_q'][keep], c['temperature'])
    assert a['n'] == len(keep) == b['n'] and abs(a['loss'] - b['loss']) <= 1e-13
    assert np.abs(a['dq'][keep] - b['dq']).max() <= 1e-14 and np.abs(a['dv'][keep] - b['dv']).max() <= 1e-14
    off = np.flatnonzero(~c['mask'])
    assert not a['dq'][off].any() and not a['dv'][off].any() and np.isnan(a['lse'][off]).all() and not a['row_loss'][off].any()


def test_a_temperature_equals_scaled_queries():
    c = O.make_case(17, 6, 'all', 8)
    t = 0.37
    a = _oracle(c, temperature=t)
    b = _oracle(c, temperature=1.0, query=c['query'].astype(np.float64) / t)
    assert abs(a['loss'] - b['loss']) <= 1e-12 and np.abs(a['dv'] - b['dv']).max() <= 1e-12
    assert np.abs(a['dq'] - b['dq'] / t).max() <= 1e-12           # d / d query = (d / d (query / t)) / t


def test_a_row_permutation_permutes_the_outputs():
    c = O.make_case(21, 5, 'all', 8)
    perm = np.random.default_rng(2).permutation(21)
    a = _oracle(c)
    b = O.in_batch_softmax_oracle(c['query'][perm], c['item'][perm], c['item_ids'][perm], c['log_q'][perm], c['temperature'], c['mask'][perm])
    assert abs(a['loss'] - b['loss']) <= 1e-13 and np.allclose(a['row_loss'][perm], b['row_loss'], rtol=0, atol=1e-13)
    assert np.abs(a['dq'][perm] - b['dq']).max() <= 1e-14 and np.abs(a['dv'][perm] - b['dv']).max() <= 1e-14


def test_every_taking_part_row_sums_p_minus_delta_to_zero():
    c = O.make_case(33, 4, 'all', 8)
    a = _oracle(c)
    on = c['mask']
    assert np.abs(a['p'][on].sum(axis=1) - 1.0).max() <= 1e-14 and not a['p'][~on].any()
    one = _oracle(c, item_ids=np.zeros(33, dtype=np.int64))      # every row its own only candidate
    assert not one['row_loss'].any() and not one['dq'].any() and not one['dv'].any() and one['loss'] == 0.0


# ---- the module without a GPU ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    q, v = torch.zeros(4, 3), torch.zeros(4, 3)
    f = M.in_batch_softmax_loss
    for bad in (lambda: f(torch.zeros(4), v), lambda: f(q, torch.zeros(4, 3, 1)), lambda: f(q, torch.zeros(4, 2)), lambda: f(q, torch.zeros(5, 3)),
                lambda: f(q, v, item_ids=torch.zeros(3, dtype=torch.int64)), lambda: f(q, v, log_q=torch.zeros(5)),
                lambda: f(q, v, mask=torch.ones(2, 4)), lambda: f(q, v, temperature=0), lambda: f(q, v, temperature=-1.0),
                lambda: f(q, v, temperature=float('nan')), lambda: f(q, v, temperature=float('inf')),
                lambda: f(q, v, item_ids=torch.zeros(4)), lambda: M.in_batch_softmax_terms(q, v, temperature=0.0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        f(torch.zeros(4, 129), torch.zeros(4, 129))
    with pytest.raises(ValueError):                    # the argument checks come first
        f(torch.zeros(4, 129), torch.zeros(4, 129), temperature=0)


def test_cpu_tensors_are_refused_after_the_argument_checks():
    q, v = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_softmax_loss(q, v, item_ids=torch.zeros(4, 1, dtype=torch.int32), log_q=torch.zeros(4, 1), mask=torch.ones(4))
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_softmax_terms(q, v)


def test_an_empty_batch_is_loss_zero_with_empty_gradients_and_no_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', boom)
    monkeypatch.setattr(_lib, 'load', boom)
    q, v = torch.zeros(0, 8, requires_grad=True), torch.zeros(0, 8, requires_grad=True)
    loss, n = M.in_batch_softmax_loss(q, v, item_ids=torch.zeros(0, dtype=torch.int64), return_num_rows=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.item() == 0.0 and n.item() == 0.0
    loss.backward()
    assert q.grad.shape == (0, 8) and v.grad.shape == (0, 8)
    t = M.in_batch_softmax_terms(q.detach(), v.detach())
    assert t.row_lse.shape == (0,) and t.row_lse.dtype == torch.float64 and t.n_rows.item() == 0.0


def test_abi_and_host_only_entry_points():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 29 and lib.recnow_abi_version() >= 29
    assert all(lib.recnow_ibs_supported(B, D) == 1 for B in (0, 1, 65536) for D in (1, 3, 127, 128))
    assert all(lib.recnow_ibs_supported(B, D) == 0 for B, D in ((4, 0), (4, 129), (-1, 8)))
    rows, tile, granule = (lib.recnow_ibs_tile(w) for w in range(3))
    assert rows >= tile >= 32 and rows % tile == 0 and granule in (2, 4, 8, 16, 32) and lib.recnow_ibs_tile(3) < 0
    assert M.MAX_D == 128


def test_the_workspace_is_the_formula():
    """16 bytes (an fp64 sum and an fp64 count) per workgroup of the forward, nothing for the backward: O(B), whatever D."""
    lib = _lib.load()
    rows = lib.recnow_ibs_tile(0)
    for B in (0, 1, rows - 1, rows, rows + 1, 600, 4096, 65536, 1 << 20):
        for D in (1, 33, 128):
            assert lib.recnow_ibs_workspace_bytes(B, D, 0) == 16 * ((B + rows - 1) // rows)
            assert lib.recnow_ibs_workspace_bytes(B, D, 1) == 0
    # the calls themselves refuse what they do not support, before anything is launched
    assert lib.recnow_ibs_fwd(None, 0, None, 0, None, None, None, 4, 129, 1.0, 1, None, None, None, None, None, None, None, 0, None) == -3
    assert lib.recnow_ibs_bwd(None, 0, None, 0, None, None, None, 4, 0, 1.0, 1, None, None, None, None, None, 0, None, 0, None, 0, None) == -1
    assert lib.recnow_ibs_fwd(None, 0, None, 0, None, None, None, 0, 8, 1.0, 1, None, None, None, None, None, None, None, 0, None) == 0

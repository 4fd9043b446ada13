"""CPU: the fp64 oracle of the in-batch sampled softmax with extra negatives (tests/_in_batch_softmax_extra_oracle.py) pinned to a hand-worked
example, to torch fp64 autograd of the (B, B + N) composition and to the oracle of the square loss; its defining properties; and everything
of the `extra_*` arguments of rec_now_amd.rec_block.in_batch_softmax that needs no GPU: argument errors, the CPU refusal, the B = 0 path, the
host-only entry points of the library, and the fp32 composition against the bounds of the GPU tests on their shapes."""
import functools
import math

import numpy as np
import pytest
import torch

import _in_batch_softmax_extra_oracle as X
import _in_batch_softmax_oracle as O
from rec_now_amd import _lib
from rec_now_amd.rec_block import in_batch_softmax as M

LSE_TOL, LOSS_TOL, GRAD_TOL = 1e-6, 1e-5, 1e-5         # the bounds of tests/test_in_batch_softmax_extra_gpu.py


def _tt(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or not t.is_floating_point() else t.to(dtype)


def test_a_hand_worked_example():
    """B = 2, N = 1, D = 2, tau = 1: logits [[1, 0 | 1], [0, 1 | 1]]."""
    q = np.array([[1., 0.], [0., 1.]])
    v = np.array([[1., 0.], [0., 1.]])
    x = np.array([[1., 1.]])
    r = X.in_batch_softmax_extra_oracle(q, v, x)
    e = math.e
    z = 2 * e + 1
    l0 = math.log(z) - 1
    assert np.allclose(r['row_loss'], [l0, l0], rtol=1e-14, atol=0) and r['n'] == 2 and abs(r['loss'] - l0) <= 1e-15
    p00, p01, p0x = e / z, 1 / z, e / z
    assert np.allclose(r['p'], [[p00, p01, p0x], [p01, p00, p0x]], rtol=1e-14, atol=0)
    assert np.allclose(r['dq'][0], [(p00 - 1 + p0x) / 2, (p01 + p0x) / 2], rtol=1e-14, atol=0)
    assert np.allclose(r['dv'][0], [(p00 - 1) / 2, p01 / 2], rtol=1e-14, atol=0)
    assert np.allclose(r['de'][0], [p0x / 2, p0x / 2], rtol=1e-14, atol=0)
    # extra_log_q = log(1/2) with log_q = 0: the extra's logit is 1 + ln 2
    r = X.in_batch_softmax_extra_oracle(q, v, x, log_q=np.zeros(2), extra_log_q=np.log([0.5]))
    assert abs(r['row_loss'][0] - (math.log(3 * e + 1) - 1)) <= 1e-15
    # the extra carries row 0's id: row 0 loses it, row 1 keeps it; it is nobody's positive
    r = X.in_batch_softmax_extra_oracle(q, v, x, item_ids=[5, 6], extra_item_ids=[5])
    assert abs(r['row_loss'][0] - (math.log(e + 1) - 1)) <= 1e-15 and abs(r['row_loss'][1] - l0) <= 1e-15 and r['p'][0, 2] == 0
    assert np.allclose(r['de'][0], [0.0, p0x / 2], rtol=1e-14, atol=0)
    # masked: the square loss
    r = X.in_batch_softmax_extra_oracle(q, v, x, extra_mask=[0])
    assert abs(r['row_loss'][0] - (math.log(e + 1) - 1)) <= 1e-15 and not r['de'].any()


@pytest.mark.parametrize('config', X.CONFIGS)
@pytest.mark.parametrize('B,N,D', [(1, 1, 3), (7, 4, 5), (41, 37, 16)])
def test_the_oracle_is_torch_fp64_autograd_of_the_composition(B, N, D, config):
    c = X.make_extra_case(B, N, D, config, 16, 8)
    r = X.oracle_of(c)
    q, v, x = (_tt(c[k]).double().requires_grad_(True) for k in ('query', 'item', 'extra_item'))
    on = np.ones(B, dtype=bool) if c['mask'] is None else c['mask']
    loss, lse, pos = X.composition_extra(q, v, x, _tt(c['item_ids']), _tt(c['log_q'], torch.float64), c['temperature'], _tt(c['mask']),
                                         _tt(c['extra_item_ids']), _tt(c['extra_log_q'], torch.float64), _tt(c['extra_mask']))
    if not on.any():
        assert r['loss'] == 0.0 and r['n'] == 0 and not r['dq'].any() and not r['dv'].any() and not r['de'].any()
        return
    gq, gv, gx = torch.autograd.grad(loss, [q, v, x])
    assert abs(r['loss'] - loss.item()) <= 1e-12 and r['n'] == on.sum()
    assert np.abs(r['dq'] - gq.numpy()).max() <= 1e-12 and np.abs(r['dv'] - gv.numpy()).max() <= 1e-12
    assert np.abs(r['de'] - gx.numpy()).max() <= 1e-12
    assert np.abs(lse.detach().numpy()[on] - r['lse'][on]).max() <= 1e-12 and np.abs(pos.detach().numpy()[on] - r['pos'][on]).max() <= 1e-12


@pytest.mark.parametrize('config', X.CONFIGS)
def test_no_extras_is_the_oracle_of_the_square_loss(config):
    c = X.make_extra_case(23, 0, 6, config, 8)
    a = X.oracle_of(c)
    b = O.in_batch_softmax_oracle(c['query'], c['item'], c['item_ids'], c['log_q'], c['temperature'], c['mask'])
    assert a['loss'] == b['loss'] and a['n'] == b['n'] and a['de'].shape == (0, 6)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ('lse', 'pos', 'row_loss', 'dq', 'dv', 'p'))


@pytest.mark.parametrize('config', X.CONFIGS)
def test_extras_are_appended_rows_with_zero_queries(config):
    """The equivalence with the square loss that holds.  Appended as rows that do NOT take part, the extras' columns would be no candidates
    either (a masked row is out on both sides).  Appended as rows that DO take part wherever extra_mask is on, with ZERO queries, every
    original row sees exactly the candidates it has with extras -- so lse, pos and p are equal -- while the appended rows themselves add
    n_x = sum(extra_mask) rows to the mean and, their queries being zero, nothing to any dv.  So with n' = n + n_x:
    lse_i, pos_i equal;  n' dq'_i = n dq_i;  n' dv'_j = n dv_j (j < B);  n' dv'_{B+k} = n de_k."""
    B, N, D = 29, 21, 5
    c = X.make_extra_case(B, N, D, config, 8, 8)
    a = X.oracle_of(c)
    on = np.ones(B, dtype=bool) if c['mask'] is None else c['mask']
    xon = np.ones(N, dtype=bool) if c['extra_mask'] is None else c['extra_mask']
    cat = lambda u, w: None if u is None else np.concatenate([u, w])      # noqa: E731
    b = O.in_batch_softmax_oracle(np.concatenate([c['query'], np.zeros((N, D), np.float32)]), np.concatenate([c['item'], c['extra_item']]),
                                  cat(c['item_ids'], c['extra_item_ids']), cat(c['log_q'], c['extra_log_q']), c['temperature'],
                                  np.concatenate([on, xon]))
    n, n2 = a['n'], b['n']
    assert n2 == n + xon.sum() and n > 0
    assert np.abs(a['lse'][on] - b['lse'][:B][on]).max() <= 1e-13 and np.abs(a['pos'][on] - b['pos'][:B][on]).max() <= 1e-13
    assert np.abs(a['p'][on] - b['p'][:B][on]).max() <= 1e-14
    assert np.abs(n * a['dq'] - n2 * b['dq'][:B]).max() <= 1e-13 and np.abs(n * a['dv'] - n2 * b['dv'][:B]).max() <= 1e-13
    assert np.abs(n * a['de'] - n2 * b['dv'][B:]).max() <= 1e-13
    assert not a['de'][~xon].any()


def test_a_permutation_of_the_extras_permutes_de_and_nothing_else():
    c = X.make_extra_case(21, 17, 5, 'all', 8, 8)
    perm = np.random.default_rng(2).permutation(17)
    a = X.oracle_of(c)
    b = X.oracle_of(c, **{k: c[k][perm] for k in ('extra_item',) + X.EXTRA_KEYS})
    assert abs(a['loss'] - b['loss']) <= 1e-13 and np.allclose(a['row_loss'], b['row_loss'], rtol=0, atol=1e-13)
    assert np.abs(a['dq'] - b['dq']).max() <= 1e-14 and np.abs(a['dv'] - b['dv']).max() <= 1e-14
    assert np.abs(a['de'][perm] - b['de']).max() <= 1e-14 and a['de'].any()


def test_a_constant_added_to_both_log_q_changes_nothing():
    c = X.make_extra_case(23, 11, 6, 'all', 8, 8)
    a = X.oracle_of(c)
    b = X.oracle_of(c, log_q=c['log_q'].astype(np.float64) + 3.25, extra_log_q=c['extra_log_q'].astype(np.float64) + 3.25)
    assert abs(a['loss'] - b['loss']) <= 1e-12
    assert all(np.abs(a[k] - b[k]).max() <= 1e-13 for k in ('dq', 'dv', 'de'))
    one = X.oracle_of(c, extra_log_q=c['extra_log_q'].astype(np.float64) + 3.25)          # one side alone is a bias
    assert abs(a['loss'] - one['loss']) > 1e-3


def test_every_taking_part_row_sums_p_to_one_over_batch_and_extras():
    c = X.make_extra_case(33, 19, 4, 'all', 8, 8)
    a = X.oracle_of(c)
    on = c['mask']
    assert np.abs(a['p'][on].sum(axis=1) - 1.0).max() <= 1e-14 and not a['p'][~on].any()
    assert a['p'][on][:, 33:].sum() > 0.05 * on.sum()              # and the extras hold a real share of it
    # every other row a hit and every extra a hit or masked: each row its own only candidate
    one = X.oracle_of(c, item_ids=np.zeros(33, dtype=np.int64), extra_item_ids=np.zeros(19, dtype=np.int64))
    assert not one['row_loss'].any() and not one['dq'].any() and not one['dv'].any() and not one['de'].any() and one['loss'] == 0.0


# ---- the module without a GPU ---------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    i4, i5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int32)
    f = M.in_batch_softmax_loss
    for bad in (lambda: f(q, v, extra_item=torch.zeros(5)), lambda: f(q, v, extra_item=torch.zeros(5, 3, 1)),          # rank
                lambda: f(q, v, extra_item=torch.zeros(5, 2)), lambda: f(q, v, extra_item=torch.zeros(5, 4)),          # D
                lambda: f(q, v, item_ids=i4, extra_item=x, extra_item_ids=torch.zeros(4, dtype=torch.int64)),          # element counts
                lambda: f(q, v, log_q=torch.zeros(4), extra_item=x, extra_log_q=torch.zeros(6)),
                lambda: f(q, v, extra_item=x, extra_mask=torch.ones(4)),
                lambda: f(q, v, item_ids=i4, extra_item=x, extra_item_ids=torch.zeros(5)),                             # float ids
                lambda: f(q, v, item_ids=i4, extra_item=x), lambda: f(q, v, extra_item=x, extra_item_ids=i5),          # half a pair
                lambda: f(q, v, log_q=torch.zeros(4), extra_item=x), lambda: f(q, v, extra_item=x, extra_log_q=torch.zeros(5)),
                lambda: f(q, v, extra_item_ids=i5), lambda: f(q, v, extra_log_q=torch.zeros(5)),                       # without extra_item
                lambda: f(q, v, extra_mask=torch.ones(5)),
                lambda: M.in_batch_softmax_terms(q, v, extra_item=torch.zeros(5, 2)),
                lambda: M.in_batch_softmax_terms(q, v, extra_mask=torch.ones(5))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        f(torch.zeros(4, 129), torch.zeros(4, 129), extra_item=torch.zeros(5, 129))
    with pytest.raises(TypeError):                     # keyword-only
        f(q, v, None, None, 1.0, None, True, False, x)


def test_cpu_tensors_are_refused_after_the_argument_checks():
    q, v, x = torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(5, 3)
    kw = dict(item_ids=torch.zeros(4, 1, dtype=torch.int32), log_q=torch.zeros(4, 1), extra_item=x,
              extra_item_ids=torch.zeros(5, 1, dtype=torch.int32), extra_log_q=torch.zeros(5, 1), extra_mask=torch.ones(5))
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_softmax_loss(q, v, **kw)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        M.in_batch_softmax_terms(q, v, extra_item=x)
    with pytest.raises(ValueError):                    # the argument checks come first
        M.in_batch_softmax_loss(q, v, **dict(kw, extra_log_q=None))


def test_an_empty_batch_with_extras_is_loss_zero_with_a_zero_de_and_no_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', boom)
    monkeypatch.setattr(_lib, 'load', boom)
    q, v = torch.zeros(0, 8, requires_grad=True), torch.zeros(0, 8, requires_grad=True)
    x = torch.full((5, 8), float('nan')).requires_grad_(True)
    loss, n = M.in_batch_softmax_loss(q, v, item_ids=torch.zeros(0, dtype=torch.int64), return_num_rows=True, extra_item=x,
                                      extra_item_ids=torch.zeros(5, dtype=torch.int64), extra_mask=torch.ones(5))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.item() == 0.0 and n.item() == 0.0
    loss.backward()
    assert q.grad.shape == (0, 8) and v.grad.shape == (0, 8) and x.grad.shape == (5, 8) and (x.grad == 0).all()
    t = M.in_batch_softmax_terms(q.detach(), v.detach(), extra_item=x.detach())
    assert t.row_lse.shape == (0,) and t.row_lse.dtype == torch.float64 and t.n_rows.item() == 0.0


def test_abi_and_host_only_entry_points():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 31 and lib.recnow_abi_version() >= 31
    assert (lib.recnow_ibs_tile(0), lib.recnow_ibs_tile(1)) == (X.R, X.T)
    assert all(lib.recnow_ibs_extra_launches(w, vec) >= 0 for w in range(4) for vec in (0, 1))
    assert all(lib.recnow_ibs_extra_launches(w, vec) < 0 for w, vec in ((-1, 0), (4, 0), (0, -1), (0, 2), (3, 2)))
    assert lib.recnow_ibs_launches(3, 0) < 0           # the square census keeps its hole


def test_the_workspace_does_not_grow_with_the_extras_and_the_calls_check_their_arguments():
    """Owners are the B queries: the forward's workspace is recnow_ibs_workspace_bytes(B, D, 0), 16 bytes per workgroup, whatever N; the
    backward's is 0.  The calls refuse bad extras before anything is launched (all pointers NULL here: nothing could run)."""
    lib = _lib.load()
    for B in (1, X.R, X.R + 1, 65536):
        assert lib.recnow_ibs_workspace_bytes(B, 64, 0) == 16 * ((B + X.R - 1) // X.R) and lib.recnow_ibs_workspace_bytes(B, 64, 1) == 0
    one = torch.zeros(1)
    p = _lib.ptr(one)

    def fwd(B=4, D=1, x=p, ldx=1, ids=None, xids=None, N=1):
        return lib.recnow_ibs_extra_fwd(p, 1, p, 1, ids, None, None, B, D, x, ldx, xids, None, None, N, 1.0, 1, None, None, None, None, None,
                                        None, None, 0, None)

    def bwd(B=4, D=1, x=p, ldx=1, ids=None, xids=None, N=1):
        return lib.recnow_ibs_extra_bwd(p, 1, p, 1, ids, None, None, B, D, x, ldx, xids, None, None, N, 1.0, 1, None, None, None, None, None, 0,
                                        None, 0, None, 0, None, 0, None)
    EINVAL, EUNSUPPORTED = -1, -3
    for f in (fwd, bwd):
        assert f(N=-1) == EINVAL and f(ldx=0) == EINVAL and f(x=None) == EINVAL and f(N=(1 << 30) + 1) == EUNSUPPORTED
        assert f(ids=p) == EINVAL and f(xids=p) == EINVAL                 # ids come in pairs
        assert f(B=-1) == EINVAL and f(D=129) == EUNSUPPORTED             # the checks of the square entries first
        assert f(B=0) == 0 and f(B=0, N=0, x=None) == 0                   # no row: nothing to do
        assert f() == EINVAL                                              # good extras, but no output pointers: refused, nothing launched


# ---- the fp32 composition against the GPU bounds, on the GPU shapes ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fractions(B, N, D, config):
    """The fraction of each GPU bound that the fp32 torch composition, run here, uses on a GPU test shape."""
    c = X.shape_case(B, N, D, config)
    r = X.oracle_of(c)
    on = np.ones(B, dtype=bool) if c['mask'] is None else c['mask']
    q, v, x = (_tt(c[k]).requires_grad_(True) for k in ('query', 'item', 'extra_item'))
    loss, lse, pos = X.composition_extra(q, v, x, _tt(c['item_ids']), _tt(c['log_q']), c['temperature'], _tt(c['mask']), _tt(c['extra_item_ids']),
                                         _tt(c['extra_log_q']), _tt(c['extra_mask']))
    out = {}
    if not on.any():
        return out
    g = torch.autograd.grad(loss, [q, v, x])
    out['loss'] = abs(loss.item() - r['loss']) / (LOSS_TOL * abs(r['loss'])) if r['loss'] != 0 else 0.0
    for what, got, want in (('row_lse', lse, r['lse']), ('row_pos_logit', pos, r['pos'])):
        out[what] = (np.abs(got.detach().double().numpy()[on] - want[on]) / (LSE_TOL * np.maximum(1.0, np.abs(want[on])))).max()
    for what, got, want in zip(('dq', 'dv', 'de'), g, (r['dq'], r['dv'], r['de'])):
        scale = np.abs(want).max(axis=1)
        nz = scale > 0
        got = got.double().numpy()
        assert np.abs(got[~nz]).max(initial=0.0) <= 1e-12
        out[what] = (np.abs(got - want)[nz].max(axis=1) / (GRAD_TOL * scale[nz])).max() if nz.any() else 0.0
    return out


@pytest.mark.parametrize('config', X.CONFIGS)
@pytest.mark.parametrize('B,N,D', X.SHAPES)
def test_the_fp32_composition_stays_under_half_of_every_gpu_bound(B, N, D, config):
    frac = _fractions(B, N, D, config)
    print(' '.join('%s %.3f' % kv for kv in sorted(frac.items())))
    assert all(f <= 0.5 for f in frac.values()), frac


def test_zz_report_the_worst_fractions_of_the_composition():
    worst = {}
    for B, N, D in X.SHAPES:
        for config in X.CONFIGS:
            for k, f in _fractions(B, N, D, config).items():
                worst[k] = max(worst.get(k, 0.0), float(f))
    for k in sorted(worst):
        print('fp32 composition, worst %-14s %.3f of the bound' % (k, worst[k]))
    assert all(f <= 0.5 for f in worst.values())

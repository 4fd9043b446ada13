"""GPU: the `extra_*` arguments of in_batch_softmax_loss / in_batch_softmax_terms (recnow_ibs_extra_*, csrc/in_batch_softmax.hip) against the
fp64 per-candidate oracle tests/_in_batch_softmax_extra_oracle.py.

Bounds (those of tests/test_in_batch_softmax_gpu.py):
  n_rows                      exact
  row_lse, row_pos_logit      |d - ref| <= 1e-6 * max(1, |ref|); NaN where the row does not take part
  row_loss                    |d - ref| <= 2e-6 * max(1, |lse|, |pos|): the difference of the two above, each inside its bound
  loss                        |d - ref| <= 1e-5 * |ref|
  dq, dv, de                  for EVERY row: max_d |d - ref| <= 1e-5 * max_d |ref| of that row; a row whose oracle gradient is 0 exactly 0
Shapes (B, N, D) come from recnow_ibs_tile: R rows owned by a workgroup, T rows of a streamed tile.  The fp32 torch composition holds every
bound with less than half of it on these inputs (tests/test_in_batch_softmax_extra_cpu.py asserts that); test_zz prints the worst fraction
seen here."""
import functools

import numpy as np
import pytest
import torch

import _in_batch_softmax_extra_oracle as X
from rec_now_amd import _lib

pytestmark = pytest.mark.gpu
LSE_TOL, LOSS_TOL, GRAD_TOL = 1e-6, 1e-5, 1e-5
WORST = {}
R, T, G = (_lib.load().recnow_ibs_tile(w) for w in range(3))
assert (R, T) == (X.R, X.T)
XKW = ('extra_item_ids', 'extra_log_q', 'extra_mask')


def _mod():
    from rec_now_amd.rec_block import in_batch_softmax as M
    return M


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _ref(B, N, D, config):
    case = X.shape_case(B, N, D, config)
    return case, X.oracle_of(case)


def _kw(case, dev):
    kw = dict(item_ids=_t(case['item_ids'], dev), log_q=_t(case['log_q'], dev), temperature=case['temperature'], mask=_t(case['mask'], dev))
    kw.update({k: _t(case[k], dev) for k in XKW})
    return kw


def _run(case, dev, q=None, v=None, x=None, gout=None, freeze=(), **over):
    """(loss, n_rows, dq, dv, de, terms) of one case; q / v / x: ready-made device tensors instead of the case's; freeze: names of the
    tensors that do not require grad (their gradient is None)."""
    M = _mod()
    q = (_t(case['query'], dev) if q is None else q).detach().requires_grad_('query' not in freeze)
    v = (_t(case['item'], dev) if v is None else v).detach().requires_grad_('item' not in freeze)
    x = (_t(case['extra_item'], dev) if x is None else x).detach().requires_grad_('extra_item' not in freeze)
    kw = _kw(case, dev)
    kw.update(over)
    loss, n = M.in_batch_softmax_loss(q, v, return_num_rows=True, extra_item=x, **kw)
    wanted = [t for t in (q, v, x) if t.requires_grad]
    grads = iter(torch.autograd.grad(loss, wanted, gout))
    dq, dv, de = (next(grads) if t.requires_grad else None for t in (q, v, x))
    return loss, n, dq, dv, de, M.in_batch_softmax_terms(q.detach(), v.detach(), extra_item=x.detach(), **kw)


def _worst(what, frac):
    WORST[what] = max(WORST.get(what, 0.0), float(frac))


def _hold_rows(what, got, want, on, tol):
    """lse / pos: inside tol * max(1, |ref|) on the taking-part rows, NaN on the others."""
    got = got.detach().cpu().double().numpy()
    assert np.isnan(got[~on]).all(), what
    if on.any():
        frac = np.abs(got[on] - want[on]) / (tol * np.maximum(1.0, np.abs(want[on])))
        print('%s: worst %.3f of the bound' % (what, frac.max()))
        _worst(what, frac.max())
        assert frac.max() <= 1.0, '%s: %.3f of the bound at row %d' % (what, frac.max(), np.flatnonzero(on)[frac.argmax()])


def _hold_grad(what, got, want):
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape
    scale = np.abs(want).max(axis=1)
    zero = scale == 0.0
    assert (got[zero] == 0.0).all(), '%s: a row whose gradient is 0 is not exactly 0' % what
    if (~zero).any():
        frac = np.abs(got - want)[~zero].max(axis=1) / (GRAD_TOL * scale[~zero])
        print('%s: worst row %.3f of the bound' % (what, frac.max()))
        _worst(what, frac.max())
        assert frac.max() <= 1.0, '%s: %.3f of the bound at row %d' % (what, frac.max(), np.flatnonzero(~zero)[frac.argmax()])


def _hold_all(got, ref, mask):
    loss, n, dq, dv, de, terms = got
    B = ref['lse'].shape[0]
    on = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    assert n.item() == ref['n'] and terms.n_rows.item() == ref['n'] and n.dtype == torch.float32
    assert loss.dim() == 0 and loss.dtype == torch.float32 and terms.row_lse.dtype == torch.float64
    _hold_rows('row_lse', terms.row_lse, ref['lse'], on, LSE_TOL)
    _hold_rows('row_pos_logit', terms.row_pos_logit, ref['pos'], on, LSE_TOL)
    rl = terms.row_loss.detach().cpu().double().numpy()
    assert (rl[~on] == 0.0).all()
    if on.any():
        bound = 2 * LSE_TOL * np.maximum(1.0, np.maximum(np.abs(ref['lse'][on]), np.abs(ref['pos'][on])))
        assert (np.abs(rl[on] - ref['row_loss'][on]) <= bound).all()
        err, bound = abs(loss.item() - ref['loss']), LOSS_TOL * abs(ref['loss'])
        assert err <= bound, 'loss %.9g against %.9g' % (loss.item(), ref['loss'])
        if bound > 0:
            print('loss: %.3f of the bound' % (err / bound))
            _worst('loss', err / bound)
    else:
        assert loss.item() == 0.0
    _hold_grad('dq', dq, ref['dq'])
    _hold_grad('dv', dv, ref['dv'])
    _hold_grad('de', de, ref['de'])


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int64 if a.dtype == torch.float64 else torch.int32)


def _same(a, b, skip=()):
    """Every output bit of two _run results equal (NaNs included); skip: positions left out (a gradient one of the runs does not have)."""
    flat = lambda r: [x for i, x in enumerate(r[:5]) if i not in skip and x is not None] + list(r[5])      # noqa: E731
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(fa, fb))


def _census():
    lib = _lib.load()
    return {('x', w, vec): lib.recnow_ibs_extra_launches(w, vec) for w in range(4) for vec in (0, 1)} | \
           {('sq', o, vec): lib.recnow_ibs_launches(o, vec) for o in (0, 1, 2) for vec in (0, 1)}


def _launched(before, kind, which):
    """Launches since `before` of one orientation, both access widths together."""
    now = _census()
    return sum(now[(kind, which, vec)] - before[(kind, which, vec)] for vec in (0, 1))


# ---- the oracle on every shape and configuration ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', X.CONFIGS)
@pytest.mark.parametrize('B,N,D', X.SHAPES)
def test_matches_the_oracle(dev, B, N, D, config):
    case, ref = _ref(B, N, D, config)
    if config in ('ids', 'all') and B >= T and N >= T:     # accidental hits among the extras, for every full workgroup of rows
        live = ref['p'].sum(axis=1) > 0
        xon = np.ones(N, dtype=bool) if case['extra_mask'] is None else case['extra_mask']
        hits = (case['item_ids'][:, None] == case['extra_item_ids'][None, :]) & live[:, None] & xon[None, :]
        assert not ref['p'][:, B:][hits].any()
        assert all(hits[r0:r0 + R].any() for r0 in range(0, B - R + 1, R) if live[r0:r0 + R].any())
    if config in ('mask', 'all') and N > T:
        assert not case['extra_mask'][:T].any() and case['extra_mask'][T:].any() and not ref['de'][:T].any()
    if config in ('plain', 'log_q'):
        assert ref['de'].all() and ref['p'][:, B:].all()
    _hold_all(_run(case, dev), ref, case['mask'])


def _big_logit_case():
    """Logits of magnitude 100 from exactly representable inputs: entries +-1/4 in D = 16 (every dot product a multiple of 1/8, times
    1 / 0.01 = 100 exact in fp32), all items and extras distinct, query_i = extra_c(i) with c a bijection: row i's maximum (100, every other
    logit <= 87.5, the positive included) stands at extra c(i), which visits every position of an extras tile and the last, ragged tile."""
    B = N = 2 * T + 5
    D = 16
    rng = np.random.default_rng(5)
    rows = (rng.integers(0, 2, (B + N, D)) * 2 - 1).astype(np.float32) / 4
    assert len({r.tobytes() for r in rows}) == B + N
    item, extra = rows[:B], rows[B:]
    c = (np.arange(B) * 5 + 3) % N
    case = dict(query=extra[c].copy(), item=item, extra_item=extra, item_ids=None, log_q=None, mask=None, temperature=0.01,
                extra_item_ids=None, extra_log_q=None, extra_mask=None)
    return case, c


@pytest.mark.parametrize('with_ids', [False, True], ids=['plain', 'ids'])
def test_logits_of_magnitude_100_do_not_overflow(dev, with_ids):
    case, c = _big_logit_case()
    B = N = len(c)
    if with_ids:
        case['item_ids'], case['extra_item_ids'] = (np.arange(B) // 3).astype(np.int32), (np.arange(N)[::-1] // 3).astype(np.int32)
        case['log_q'], case['extra_log_q'] = (np.arange(B) % 4).astype(np.float32), (np.arange(N) % 3).astype(np.float32)
    ref = X.oracle_of(case)
    if not with_ids:
        top = ref['p'].argmax(axis=1) - B
        assert (top == c).all() and set(top % T) == set(range(T)) and (top >= 2 * T).any()
        assert abs(ref['lse']).max() >= 100 and abs(ref['pos']).max() <= 87.5
    got = _run(case, dev)
    assert torch.isfinite(got[0]) and all(torch.isfinite(g).all() for g in got[2:5])
    _hold_all(got, ref, None)


@pytest.mark.parametrize('B,N', [(1, 3), (R + 3, T + 7)])
def test_a_row_whose_extras_are_all_hits_or_masked_has_loss_zero_and_zero_gradient(dev, B, N):
    case = X.make_extra_case(B, N, 33, 'log_q', R, T, seed=1)
    case['item_ids'] = np.full(B, 11, dtype=np.int64)                   # every other row is an accidental hit,
    case['extra_item_ids'] = np.where(np.arange(N) % 2 == 0, 11, 12).astype(np.int64)     # every second extra too,
    case['extra_mask'] = np.arange(N) % 2 == 0                          # and the others are masked
    loss, n, dq, dv, de, terms = _run(case, dev)
    assert loss.item() == 0.0 and n.item() == B
    assert (dq == 0).all() and (dv == 0).all() and (de == 0).all() and (terms.row_loss == 0).all()
    assert torch.equal(terms.row_lse, terms.row_pos_logit.double())     # lse_i == s_ii bit for bit
    if B > 1:                                                           # one live extra: every row gains a loss, and only that extra a gradient
        case['extra_item_ids'][0] = 12
        got = _run(case, dev)
        assert got[0].item() > 0.0 and (got[5].row_loss > 0).all() and (got[4][1:] == 0).all() and (got[4][0] != 0).any()
        _hold_all(got, X.oracle_of(case), None)


def test_masked_extras_full_of_nan_and_inf_touch_no_bit(dev):
    B, N, D = 129, 97, 128
    case, _ = _ref(B, N, D, 'all')
    off = ~case['extra_mask']
    fill = np.where(np.arange(D) % 3 == 0, np.nan, np.where(np.arange(D) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    outs = []
    for bad in (False, True):
        c = dict(case, extra_item=case['extra_item'].copy(), extra_log_q=case['extra_log_q'].copy())
        c['extra_item'][off] = fill if bad else 0.25
        outs.append(_run(c, dev))
    assert off.sum() > T and _same(outs[0], outs[1]) and torch.isfinite(outs[1][0])
    assert (outs[1][4][torch.from_numpy(off).to(dev)] == 0).all()


def test_a_nan_in_an_unmasked_extra_makes_the_loss_nan(dev):
    case, _ = _ref(65, 1, 64, 'plain')
    c = dict(case, extra_item=case['extra_item'].copy())
    c['extra_item'][0, 5] = np.nan
    assert torch.isnan(_run(c, dev)[0])
    case, _ = _ref(197, 129, 64, 'mask')
    c = dict(case, extra_item=case['extra_item'].copy())
    c['extra_item'][np.flatnonzero(case['extra_mask'])[-1], 63] = np.nan
    assert torch.isnan(_run(c, dev)[0])


@pytest.mark.parametrize('B,N,D', [(197, 129, 64), (64, 33, 33)])
def test_a_row_strided_view_and_an_offset_storage_give_the_aligned_bits(dev, B, N, D):
    case, _ = _ref(B, N, D, 'all')
    want = _run(case, dev)
    for col in (4, 1):                                 # a column slice of a wider tower output; col 1: the storage is off by one float
        wide = torch.full((N, D + 12), 7.0, device=dev)
        wide[:, col:col + D] = _t(case['extra_item'], dev)
        before = _census()
        got = _run(case, dev, x=wide[:, col:col + D])
        assert _same(want, got)
        if D == 64:                                    # the view itself reached the kernels: guarded accesses for col 1 (a copy would be aligned)
            now = _census()
            vec = 1 if col == 4 else 0
            assert all(now[('x', w, vec)] > before[('x', w, vec)] and now[('x', w, 1 - vec)] == before[('x', w, 1 - vec)] for w in (0, 1, 2))
            assert now[('x', 3, 1)] > before[('x', 3, 1)]              # the queries stayed aligned
    xt = _t(case['extra_item'].T.copy(), dev).T        # column-major: made contiguous, same bits
    assert _same(want, _run(case, dev, x=xt))


def test_census_every_access_width_in_every_orientation(dev):
    lib = _lib.load()
    before = _census()
    for B, N, D in ((65, 1, 64), (2, 31, 3)):
        _run(_ref(B, N, D, 'plain')[0], dev)
    now = _census()
    # a _run is two forwards (the loss, the terms) and one backward; the first shape takes 16-byte accesses throughout, the second none
    assert all(now[('x', w, vec)] == before[('x', w, vec)] + (2 if w == 0 else 1) for w in range(4) for vec in (0, 1))
    assert lib.recnow_ibs_extra_launches(4, 0) < 0 and lib.recnow_ibs_extra_launches(0, 2) < 0 and lib.recnow_ibs_extra_launches(-1, 0) < 0
    case, _ = _ref(65, 1, 64, 'plain')                 # the queries' width is which 3's own: an offset query storage, aligned extras
    wide = torch.zeros((65, 80), device=dev)
    wide[:, 1:65] = _t(case['query'], dev)
    before = _census()
    _run(case, dev, q=wide[:, 1:65])
    now = _census()
    assert now[('x', 3, 0)] == before[('x', 3, 0)] + 1 and now[('x', 2, 1)] == before[('x', 2, 1)] + 1


def test_a_frozen_extra_item_launches_no_de(dev):
    case, _ = _ref(129, 97, 128, 'all')
    full = _run(case, dev)
    before = _census()
    frozen = _run(case, dev, freeze=('extra_item',))
    assert _launched(before, 'x', 1) == 1 and _launched(before, 'sq', 2) == 1
    assert _launched(before, 'x', 2) == 0 and _launched(before, 'x', 3) == 0 and frozen[4] is None
    assert _same(full, frozen, skip=(4,))


def test_frozen_towers_with_a_trainable_extra_item_launch_de_only(dev):
    case, _ = _ref(129, 97, 128, 'all')
    full = _run(case, dev)
    before = _census()
    only = _run(case, dev, freeze=('query', 'item'))
    assert _launched(before, 'x', 2) == 1 and _launched(before, 'x', 3) == 1
    assert _launched(before, 'x', 1) == 0 and all(_launched(before, 'sq', o) == 0 for o in (0, 1, 2))
    assert only[2] is None and only[3] is None and _same(full, only, skip=(2, 3))


@pytest.mark.parametrize('config', ['plain', 'all'])
def test_no_extras_rows_is_the_call_without_extras_bit_for_bit(dev, config):
    M = _mod()
    case, _ = _ref(197, 129, 64, config)
    kw = {k: v for k, v in _kw(case, dev).items() if k not in XKW}
    outs = []
    for with_extras in (False, True):
        q, v = (_t(case[k], dev).requires_grad_(True) for k in ('query', 'item'))
        x = torch.zeros((0, 64), device=dev, requires_grad=True)
        xkw = {}
        if with_extras:
            xkw = dict(extra_item=x, extra_mask=torch.zeros(0, device=dev))
            if case['item_ids'] is not None:
                xkw.update(extra_item_ids=torch.zeros(0, dtype=torch.int64, device=dev), extra_log_q=torch.zeros(0, device=dev))
        before = _census()
        loss, n = M.in_batch_softmax_loss(q, v, return_num_rows=True, **kw, **xkw)
        grads = torch.autograd.grad(loss, [q, v, x] if with_extras else [q, v])
        terms = M.in_batch_softmax_terms(q.detach(), v.detach(), **kw, **xkw)
        assert all(_launched(before, 'x', w) == 0 for w in range(4))
        assert _launched(before, 'sq', 0) == 2 and _launched(before, 'sq', 1) == 1 and _launched(before, 'sq', 2) == 1
        if with_extras:
            assert grads[2].shape == (0, 64) and grads[2].dtype == torch.float32
        outs.append([loss, n, grads[0], grads[1]] + list(terms))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)) and torch.isfinite(outs[0][0])


def test_repeated_runs_and_graph_replay_are_bit_for_bit(dev):
    M = _mod()
    case, _ = _ref(197, 129, 64, 'all')
    assert _same(_run(case, dev), _run(case, dev))
    q, v, x = (_t(case[k], dev).requires_grad_(True) for k in ('query', 'item', 'extra_item'))
    kw = _kw(case, dev)

    def step():
        loss = M.in_batch_softmax_loss(q, v, extra_item=x, **kw)
        return (loss,) + torch.autograd.grad(loss, [q, v, x])
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(9)
    for _ in range(2):
        with torch.no_grad():                          # new contents, same storage
            for t in (q, v, x):
                t.copy_(torch.from_numpy(rng.standard_normal(tuple(t.shape)).astype(np.float32) * 0.3))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, eager)) and torch.isfinite(outs[0]) and outs[3].any()


def test_the_upstream_gradient_scales_dq_dv_and_de(dev):
    case, _ = _ref(64, 33, 33, 'all')
    one = _run(case, dev)
    four = _run(case, dev, gout=torch.tensor(4.0, device=dev))          # a power of two: exact
    assert all(torch.equal(four[i], 4 * one[i]) and one[i].any() for i in (2, 3, 4))
    third = _run(case, dev, gout=torch.tensor(-1.0 / 3, device=dev))
    assert all(torch.allclose(third[i], one[i] * (-1.0 / 3), rtol=1e-6, atol=0) for i in (2, 3, 4))


def test_peak_memory_holds_no_b_by_b_plus_n_matrix(dev):
    """Forward + backward at B 1024, N 3072, D 32: above the inputs, the three gradients, O(B) outputs (64 bytes a query row, nothing per
    extra) and the workspace, with the 64 KB allowance of the square loss's test; one (B, B + N) fp32 matrix would be 16 MB."""
    M = _mod()
    lib = _lib.load()
    B, N, D = 1024, 3072, 32
    gen = torch.Generator(device='cpu').manual_seed(3)
    q, v = ((torch.randn(B, D, generator=gen) * 0.4).to(dev).requires_grad_(True) for _ in range(2))
    x = (torch.randn(N, D, generator=gen) * 0.4).to(dev).requires_grad_(True)
    ids, xids = torch.randint(0, B // 4, (B,), generator=gen).to(dev), torch.randint(0, B // 4, (N,), generator=gen).to(dev)
    lq, xlq = torch.rand(B, generator=gen).add_(0.05).log_().to(dev), torch.rand(N, generator=gen).add_(0.05).log_().to(dev)
    xm = (torch.rand(N, generator=gen) > 0.1).to(dev)

    def step():
        loss = M.in_batch_softmax_loss(q, v, item_ids=ids, log_q=lq, temperature=0.7, extra_item=x, extra_item_ids=xids, extra_log_q=xlq,
                                       extra_mask=xm)
        return (loss,) + torch.autograd.grad(loss, [q, v, x])
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = (2 * B + N) * D * 4 + 64 * B + lib.recnow_ibs_workspace_bytes(B, D, 0) + lib.recnow_ibs_workspace_bytes(B, D, 1) + 65536
    assert torch.isfinite(outs[0]) and outs[3].any()
    assert rise <= allowed < B * (B + N) * 4 // 16, 'forward + backward rose %d bytes, allowed %d' % (rise, allowed)


def test_two_dense_towers_with_sampled_items_match_fp64_autograd(dev):
    """Mixed negative sampling: the item tower runs on cat(batch items, sampled items) and its output is split.  Every module gradient within
    1e-5 of its tensor's largest entry.  The item tower's bias is the exception in scale only: a vector added to every item and extra shifts
    all logits of a row alike, so its gradient is zero identically, and it is held to 1e-5 of sum_j |dv_j| + sum_k |de_k| instead."""
    import dense_ref as Rf
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    M = _mod()
    torch.manual_seed(4)
    rng = np.random.default_rng(21)
    B, N, U = R + 9, T + 11, 16
    xu = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(dev)
    xi = torch.from_numpy(rng.standard_normal((B + N, 20)).astype(np.float32)).to(dev)
    ids = torch.from_numpy(rng.integers(0, B // 4, B + N)).to(dev)
    lq = torch.from_numpy(np.log(rng.uniform(0.05, 1.0, B + N)).astype(np.float32)).to(dev)
    tu, ti = MultiDenseLayer(U, 1), MultiDenseLayer(U, 1)
    items = ti(xi).reshape(B + N, U)
    loss = M.in_batch_softmax_loss(tu(xu).reshape(B, U), items[:B], item_ids=ids[:B], log_q=lq[:B], temperature=0.8, extra_item=items[B:],
                                   extra_item_ids=ids[B:], extra_log_q=lq[B:])
    params = [tu.kernel, tu.bias, ti.kernel, ti.bias]
    grads = torch.autograd.grad(loss, params)
    p64 = [p.detach().cpu().double().requires_grad_(True) for p in params]
    q64 = Rf.multi_dense_layer(xu.cpu().double(), p64[0], p64[1]).reshape(B, U)
    i64 = Rf.multi_dense_layer(xi.cpu().double(), p64[2], p64[3]).reshape(B + N, U)
    ids_c, lq_c = ids.cpu(), lq.cpu().double()
    ref = X.composition_extra(q64, i64[:B], i64[B:], ids_c[:B], lq_c[:B], 0.8, None, ids_c[B:], lq_c[B:])[0]
    *g64, di64 = torch.autograd.grad(ref, p64 + [i64])
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item())
    for name, got, want in zip(('user kernel', 'user bias', 'item kernel', 'item bias'), grads, g64):
        err, scale = (got.detach().cpu().double() - want).abs().max().item(), want.abs().max().item()
        if name == 'item bias':                        # sum_j dv_j + sum_k de_k = sum_i q_i (sum p_i. - 1) = 0 identically: held against its terms
            assert scale <= 1e-12
            scale = di64.abs().sum(dim=0).max().item()
        _worst('module d ' + name, err / (GRAD_TOL * scale))
        assert err <= GRAD_TOL * scale, '%s: %.3g against %.3g' % (name, err, scale)


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of each bound seen by the tests above (printed; the bounds themselves are asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())

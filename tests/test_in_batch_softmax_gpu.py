"""GPU: in_batch_softmax_loss / in_batch_softmax_terms (csrc/in_batch_softmax.hip) against the fp64 per-candidate oracle
tests/_in_batch_softmax_oracle.py.

Bounds:
  n_rows                      exact
  row_lse, row_pos_logit      |d - ref| <= 1e-6 * max(1, |ref|); NaN where the row does not take part
  row_loss                    |d - ref| <= 2e-6 * max(1, |lse|, |pos|): the difference of the two above, each inside its bound
  loss                        |d - ref| <= 1e-5 * |ref|
  dq, dv                      for EVERY row: max_d |d - ref| <= 1e-5 * max_d |ref| of that row; a row whose oracle gradient is 0 exactly 0
Shapes come from recnow_ibs_tile: R rows owned by a workgroup, T rows of a streamed tile.  The fp32 torch composition holds every bound with
less than half of it on these inputs (run on the CPU before these tests first met a GPU); test_zz prints the worst fraction seen here."""
import functools

import numpy as np
import pytest
import torch

import _in_batch_softmax_oracle as O
from rec_now_amd import _lib

pytestmark = pytest.mark.gpu
LSE_TOL, LOSS_TOL, GRAD_TOL = 1e-6, 1e-5, 1e-5
WORST = {}
R, T, G = (_lib.load().recnow_ibs_tile(w) for w in range(3))
# B: 1, 2, a tile - 1 / a tile / a tile + 1 of either side, two row tiles + 1, a ragged batch of three row tiles (and six streamed ones)
SHAPES = [(1, 1), (2, 3), (T - 1, 8), (T, 33), (T + 1, 64), (R - 1, 127), (R, 128), (R + 1, 33), (2 * R + 1, 64), (2 * R + 1, 127),
          (3 * R + 5, 3), (3 * R + 5, 128)]


def _mod():
    from rec_now_amd.rec_block import in_batch_softmax as M
    return M


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mask_tile(B):
    """The tile the 'mask' configurations remove as a whole: a workgroup's rows where the batch has three of them, else a wave's rows (which
    is also a streamed tile) -- a workgroup's would be half of the batch and more."""
    return R if B >= 3 * R else T


@functools.lru_cache(maxsize=None)
def _ref(B, D, config):
    case = O.make_case(B, D, config, _mask_tile(B))
    return case, O.in_batch_softmax_oracle(case['query'], case['item'], case['item_ids'], case['log_q'], case['temperature'], case['mask'])


def _run(case, dev, q=None, v=None, gout=None, freeze_item=False, **over):
    """(loss, n_rows, dq, dv, terms) of one case; q / v: ready-made device tensors instead of the case's."""
    M = _mod()
    q = (_t(case['query'], dev) if q is None else q).detach().requires_grad_(True)
    v = (_t(case['item'], dev) if v is None else v).detach().requires_grad_(not freeze_item)
    kw = dict(item_ids=_t(case['item_ids'], dev), log_q=_t(case['log_q'], dev), temperature=case['temperature'], mask=_t(case['mask'], dev))
    kw.update(over)
    loss, n = M.in_batch_softmax_loss(q, v, return_num_rows=True, **kw)
    grads = torch.autograd.grad(loss, [q] if freeze_item else [q, v], gout)
    return loss, n, grads[0], None if freeze_item else grads[1], M.in_batch_softmax_terms(q.detach(), v.detach(), **kw)


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
    scale = np.abs(want).max(axis=1)
    zero = scale == 0.0
    assert (got[zero] == 0.0).all(), '%s: a row whose gradient is 0 is not exactly 0' % what
    if (~zero).any():
        frac = np.abs(got - want)[~zero].max(axis=1) / (GRAD_TOL * scale[~zero])
        print('%s: worst row %.3f of the bound' % (what, frac.max()))
        _worst(what, frac.max())
        assert frac.max() <= 1.0, '%s: %.3f of the bound at row %d' % (what, frac.max(), np.flatnonzero(~zero)[frac.argmax()])


def _hold_all(got, ref, mask):
    loss, n, dq, dv, terms = got
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


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int64 if a.dtype == torch.float64 else torch.int32)


def _same(a, b):
    """Every output bit of two _run results equal (NaNs included)."""
    flat = lambda r: [r[0], r[1]] + [x for x in r[2:4] if x is not None] + list(r[4])      # noqa: E731
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(flat(a), flat(b)))


# ---- the oracle on every shape and configuration ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', O.CONFIGS)
@pytest.mark.parametrize('B,D', SHAPES)
def test_matches_the_oracle(dev, B, D, config):
    case, ref = _ref(B, D, config)
    if config in ('ids', 'all') and B >= T:            # accidental hits in every tile of rows
        live = ref['p'].sum(axis=1) > 0
        hits = (ref['p'] == 0) & (case['item_ids'][:, None] == case['item_ids'][None, :]) & live[:, None] & live[None, :]
        assert all(hits[r0:r0 + R].any() for r0 in range(0, B - R + 1, R) if live[r0:r0 + R].any())     # every full tile of rows
    if config in ('mask', 'all') and B > T:
        w = _mask_tile(B)
        assert not case['mask'][w:2 * w].any() and 0.15 < 1 - case['mask'].mean() < 0.65
    _hold_all(_run(case, dev), ref, case['mask'])


def _big_logit_case():
    """Logits of magnitude 100 from exactly representable inputs: entries +-1/4 in D = 16 (every dot product a multiple of 1/8, times 1 / 0.01 =
    100 exact in fp32), query_i = item_c(i) with c a bijection: row i's maximum (100, the others <= 87.5) stands at column c(i), which visits
    every position of a streamed tile and the last, ragged tile."""
    B, D = 2 * T + 5, 16
    rng = np.random.default_rng(5)
    item = (rng.integers(0, 2, (B, D)) * 2 - 1).astype(np.float32) / 4
    assert len({r.tobytes() for r in item}) == B
    c = (np.arange(B) * 5 + 3) % B
    return dict(query=item[c].copy(), item=item, item_ids=None, log_q=None, mask=None, temperature=0.01), c


@pytest.mark.parametrize('with_ids', [False, True], ids=['plain', 'ids'])
def test_logits_of_magnitude_100_do_not_overflow(dev, with_ids):
    case, c = _big_logit_case()
    B = len(c)
    if with_ids:
        case['item_ids'] = (np.arange(B) // 3).astype(np.int32)
        case['log_q'] = (np.arange(B) % 4).astype(np.float32)
    ref = O.in_batch_softmax_oracle(case['query'], case['item'], case['item_ids'], case['log_q'], case['temperature'])
    if not with_ids:
        top = ref['p'].argmax(axis=1)
        assert (top == c).all() and set(top % T) == set(range(T)) and (top >= 2 * T).any() and abs(ref['pos']).max() >= 100
    got = _run(case, dev)
    assert torch.isfinite(got[0]) and torch.isfinite(got[2]).all() and torch.isfinite(got[3]).all()
    _hold_all(got, ref, None)


@pytest.mark.parametrize('B', [1, R + 3])
def test_a_row_that_is_its_only_candidate_has_loss_zero_and_zero_gradient(dev, B):
    case = O.make_case(B, 33, 'log_q', R, seed=1)
    case['item_ids'] = np.full(B, 11, dtype=np.int64)                   # every other row is an accidental hit
    loss, n, dq, dv, terms = _run(case, dev)
    assert loss.item() == 0.0 and n.item() == B
    assert (dq == 0).all() and (dv == 0).all() and (terms.row_loss == 0).all()
    assert torch.equal(terms.row_lse, terms.row_pos_logit.double())     # lse_i == s_ii bit for bit
    if B > 1:                                                           # and the same through the mask: one row left
        case['item_ids'], case['mask'] = None, np.arange(B) == R + 1
        loss, n, dq, dv, terms = _run(case, dev)
        assert loss.item() == 0.0 and n.item() == 1 and (dq == 0).all() and (dv == 0).all()


def test_masked_rows_full_of_nan_and_inf_touch_no_bit(dev):
    case, _ = _ref(3 * R + 5, 128, 'all')
    off = ~case['mask']
    fill = np.where(np.arange(128) % 3 == 0, np.nan, np.where(np.arange(128) % 3 == 1, np.inf, -np.inf)).astype(np.float32)
    outs = []
    for bad in (False, True):
        c = dict(case, query=case['query'].copy(), item=case['item'].copy(), log_q=case['log_q'].copy())
        c['query'][off], c['item'][off] = (fill, fill) if bad else (0.0, 0.0)
        outs.append(_run(c, dev))
    assert _same(outs[0], outs[1]) and torch.isfinite(outs[1][0])


def test_a_nan_in_a_taking_part_row_makes_the_loss_nan(dev):
    case, _ = _ref(2 * R + 1, 64, 'mask')
    c = dict(case, item=case['item'].copy())
    c['item'][np.flatnonzero(case['mask'])[-1], 5] = np.nan
    assert torch.isnan(_run(c, dev)[0])


@pytest.mark.parametrize('D', [64, 33])
def test_row_strided_views_and_an_offset_storage_give_the_aligned_bits(dev, D):
    lib = _lib.load()
    case, _ = _ref(R + 1, 33, 'all') if D == 33 else _ref(2 * R + 1, 64, 'all')
    B = case['query'].shape[0]
    want = _run(case, dev)
    for col in (4, 1):                                 # a column slice of a wider tower output; col 1: the storage is off by one float
        wide_q, wide_v = (torch.full((B, D + 12), 7.0, device=dev) for _ in range(2))
        wide_q[:, col:col + D], wide_v[:, col:col + D] = _t(case['query'], dev), _t(case['item'], dev)
        before = [lib.recnow_ibs_launches(o, 0) for o in (0, 1, 2)]
        got = _run(case, dev, q=wide_q[:, col:col + D], v=wide_v[:, col:col + D])
        assert _same(want, got)
        if col == 1 and D == 64:                       # a contiguous copy would have been aligned: the view itself reached the kernels
            assert all(lib.recnow_ibs_launches(o, 0) > b for o, b in zip((0, 1, 2), before))
    qt = _t(case['query'].T.copy(), dev).T             # column-major: made contiguous, same bits
    assert _same(want, _run(case, dev, q=qt))


def test_census_every_access_width_in_every_orientation(dev):
    lib = _lib.load()
    before = {(o, w): lib.recnow_ibs_launches(o, w) for o in (0, 1, 2, 4, 5, 6) for w in (0, 1)}
    for B, D in ((T + 1, 64), (2, 3)):
        _run(_ref(B, D, 'plain')[0], dev)
    assert all(lib.recnow_ibs_launches(o, w) > n for (o, w), n in before.items())
    assert lib.recnow_ibs_launches(3, 0) < 0 and lib.recnow_ibs_launches(0, 2) < 0


def test_repeated_runs_and_graph_replay_are_bit_for_bit(dev):
    M = _mod()
    case, _ = _ref(3 * R + 5, 128, 'all')
    assert _same(_run(case, dev), _run(case, dev))
    q, v = _t(case['query'], dev).requires_grad_(True), _t(case['item'], dev).requires_grad_(True)
    kw = dict(item_ids=_t(case['item_ids'], dev), log_q=_t(case['log_q'], dev), temperature=case['temperature'], mask=_t(case['mask'], dev))

    def step():
        loss = M.in_batch_softmax_loss(q, v, **kw)
        return (loss,) + torch.autograd.grad(loss, [q, v])
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(9)
    for _ in range(2):
        with torch.no_grad():                          # new contents, same storage
            q.copy_(torch.from_numpy(rng.standard_normal(case['query'].shape).astype(np.float32) * 0.3))
            v.copy_(torch.from_numpy(rng.standard_normal(case['item'].shape).astype(np.float32) * 0.3))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, eager)) and torch.isfinite(outs[0])


def test_the_upstream_gradient_scales_dq_and_dv(dev):
    case, _ = _ref(R + 1, 33, 'all')
    one = _run(case, dev)
    four = _run(case, dev, gout=torch.tensor(4.0, device=dev))          # a power of two: exact
    assert torch.equal(four[2], 4 * one[2]) and torch.equal(four[3], 4 * one[3])
    third = _run(case, dev, gout=torch.tensor(-1.0 / 3, device=dev))
    for a, b in ((third[2], one[2]), (third[3], one[3])):
        assert torch.allclose(a, b * (-1.0 / 3), rtol=1e-6, atol=0)


def test_a_frozen_item_tower_launches_no_dv(dev):
    lib = _lib.load()
    case, _ = _ref(2 * R + 1, 64, 'all')
    full = _run(case, dev)
    n_dq, n_dv = (sum(lib.recnow_ibs_launches(o, w) for w in (0, 1)) for o in (1, 2))
    frozen = _run(case, dev, freeze_item=True)
    assert sum(lib.recnow_ibs_launches(1, w) for w in (0, 1)) == n_dq + 1
    assert sum(lib.recnow_ibs_launches(2, w) for w in (0, 1)) == n_dv
    assert torch.equal(frozen[0], full[0]) and torch.equal(frozen[2], full[2])


def test_peak_memory_holds_no_b_by_b_matrix(dev):
    """Forward + backward at B 4096, D 32: above the inputs, the gradients, O(B) outputs (64 bytes a row) and the workspace; one (B, B) fp32
    matrix would be 64 MB."""
    M = _mod()
    B, D = 4096, 32
    gen = torch.Generator(device='cpu').manual_seed(3)
    q = (torch.randn(B, D, generator=gen) * 0.4).to(dev).requires_grad_(True)
    v = (torch.randn(B, D, generator=gen) * 0.4).to(dev).requires_grad_(True)
    ids = torch.randint(0, B // 4, (B,), generator=gen).to(dev)
    lq = torch.rand(B, generator=gen).add_(0.05).log_().to(dev)

    def step():
        loss = M.in_batch_softmax_loss(q, v, item_ids=ids, log_q=lq, temperature=0.7)
        return (loss,) + torch.autograd.grad(loss, [q, v])
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    outs = step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = 2 * B * D * 4 + 64 * B + _lib.load().recnow_ibs_workspace_bytes(B, D, 0) + _lib.load().recnow_ibs_workspace_bytes(B, D, 1) + 65536
    assert torch.isfinite(outs[0]) and rise <= allowed < B * B * 4 // 16, 'forward + backward rose %d bytes, allowed %d' % (rise, allowed)


def test_two_dense_towers_into_the_loss_match_fp64_autograd(dev):
    """Every module gradient within 1e-5 of its tensor's largest entry.  The item tower's bias is the exception in scale only: a vector added to
    every item shifts all logits of a row alike, so its gradient is zero identically, and it is held to 1e-5 of sum_j |dv_j| instead."""
    import dense_ref as Rf
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    M = _mod()
    torch.manual_seed(4)
    rng = np.random.default_rng(21)
    B, U = R + 9, 16
    xu = torch.from_numpy(rng.standard_normal((B, 24)).astype(np.float32)).to(dev)
    xi = torch.from_numpy(rng.standard_normal((B, 20)).astype(np.float32)).to(dev)
    ids = torch.from_numpy(rng.integers(0, B // 4, B)).to(dev)
    lq = torch.from_numpy(np.log(rng.uniform(0.05, 1.0, B)).astype(np.float32)).to(dev)
    tu, ti = MultiDenseLayer(U, 1), MultiDenseLayer(U, 1)
    loss = M.in_batch_softmax_loss(tu(xu).reshape(B, U), ti(xi).reshape(B, U), item_ids=ids, log_q=lq, temperature=0.8)
    params = [tu.kernel, tu.bias, ti.kernel, ti.bias]
    grads = torch.autograd.grad(loss, params)
    p64 = [p.detach().cpu().double().requires_grad_(True) for p in params]
    q64 = Rf.multi_dense_layer(xu.cpu().double(), p64[0], p64[1]).reshape(B, U)
    v64 = Rf.multi_dense_layer(xi.cpu().double(), p64[2], p64[3]).reshape(B, U)
    ref = O.composition(q64, v64, ids.cpu(), lq.cpu().double(), 0.8)[0]
    *g64, dv64 = torch.autograd.grad(ref, p64 + [v64])
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item())
    for name, got, want in zip(('user kernel', 'user bias', 'item kernel', 'item bias'), grads, g64):
        err, scale = (got.detach().cpu().double() - want).abs().max().item(), want.abs().max().item()
        if name == 'item bias':                        # sum_j dv_j = sum_i q_i (sum_j p_ij - 1) = 0 identically: held against the terms it sums
            assert scale <= 1e-12
            scale = dv64.abs().sum(dim=0).max().item()
        _worst('module d ' + name, err / (GRAD_TOL * scale))
        assert err <= GRAD_TOL * scale, '%s: %.3g against %.3g' % (name, err, scale)


def test_zz_report_the_worst_fractions():
    """Last in the file: the largest fraction of each bound seen by the tests above (printed; the bounds themselves are asserted there)."""
    for what in sorted(WORST):
        print('worst %-24s %.3f of the bound' % (what, WORST[what]))
    assert all(v <= 1.0 for v in WORST.values())

"""GPU: listmle_loss_from_batch / listmle_terms (csrc/listmle.hip) against the fp64 per-list oracle tests/_listmle_oracle.py.

Bounds (the project's own, as in tests/test_listwise_lists_gpu.py):
  n_valid, positions, validity   exact
  lse                            |d - ref| <= 1e-12 * |ref| (fp64 end to end; the device library's fp64 log / exp are not bit-specified)
  loss, per-list losses          |d - ref| <= 1e-5 * |ref|
  gradient                       for EVERY valid list g: max_i |d_i - ref_i| <= 1e-5 * max_i |ref_i| over the rows of g; rows of invalid lists,
                                 masked rows and rows with a NaN label exactly 0; |sum_i d_i| <= 1e-5 * max_i |ref_i|
  reproducibility                the same call twice: bitwise equal
Layouts aim at the scan's tile of RECNOW_LISTMLE_TILE = 1024 positions.  The ids are int64 and ascending with the list, so list g occupies
[cum[g], cum[g + 1]) of the sorted order whatever the row order of the batch is, and `_census` restates from the sizes alone which tile classes a
layout reaches.  Logits of 'magnitude 120' are logits around +120 or -120, list by list (exp overflows fp32 there), with a spread of 1 inside a
list: at |s| = 120 the rounding of s - lse is 1.4e-14 absolute in fp64, which is above 1e-5 of a list's largest gradient entry only where that
entry is below 1e-9 -- lists whose rows differ by tens of units and already stand in label order; the oracle itself differs from
torch.logcumsumexp autograd there (tests/test_listmle_cpu.py uses the same logits)."""
import functools
import os

import numpy as np
import pytest
import torch

import _listmle_oracle as MO

pytestmark = pytest.mark.gpu
T = 1024
RTOL = 1e-5
LSE_RTOL = 1e-12


def _mod():
    from rec_now_amd.rec_block import listmle as M
    return M


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    # lists of 1 / 2 / 3 / 1023 / 1024 / 1025 / 2049 rows and one of 3000 (positions 5127 .. 8127: tiles 5, 6, 7 -- all of tile 6), then short ones
    'sizes': [1, 2, 3, 1023, 1024, 1025, 2049, 3000, 7, 1, 4, 2, 8],
    # a list boundary exactly on a tile boundary (1024), one position behind one (2049), and again on one (4096)
    'boundary': [1024, 1025, 2047, 5, 3, 1500, 6, 9],
    # many lists of 2 to 5 rows in one tile
    'packed': [2 + (i * 7) % 4 for i in range(700)] + [6, 8],
    # every row in one list
    'one_list': [2500],
    'single_row': [1],
}


def _census(sizes, n_members):
    cum = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    a, e = cum[:-1], cum[1:]
    B = int(cum[-1])
    first_tile, last_tile = a // T, (e - 1) // T
    mem_end = a + n_members
    next_edge = (a // T + 1) * T                      # the first tile boundary behind a
    return {
        'B off the tile': B % T != 0,
        'more than one tile': B > T,
        'a list over three tiles': bool(((last_tile - first_tile) >= 2).any()),
        'a list over two tiles': bool(((last_tile - first_tile) == 1).any()),
        'a list begins on a tile boundary': bool(((a % T == 0) & (a > 0)).any()),
        'a list begins one behind a tile boundary': bool((a % T == 1).any() and (a[a % T == 1] > 1).any()),
        'a hundred lists in one tile': bool(np.bincount(first_tile[first_tile == last_tile], minlength=1).max(initial=0) >= 100),
        'a tile boundary inside the rows that do not take part': bool(((mem_end < next_edge) & (next_edge < e)).any()),
        'a tile boundary inside the members behind place 3': bool(((a + 3 < next_edge) & (next_edge < mem_end)).any()),
        'lists of 1, 2 and 3 rows': all((np.asarray(sizes) == k).any() for k in (1, 2, 3)),
        'a list with no member': bool(((n_members == 0) & (np.asarray(sizes) >= 2)).any()),
    }


def _labels(rng, B, kind):
    if kind == 'levels':
        return rng.integers(0, 4, B).astype(np.float32)
    return rng.normal(size=B).astype(np.float32)


def _logits(rng, k, kind):
    s = rng.normal(size=k.size)
    if kind == 'mag120':
        s = s + 120.0 * np.where(k % 2 == 0, 1.0, -1.0)
    return s.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(layout, labels='levels', logits='unit', seed=0):
    """ids (int64, ascending with the list), labels, logits, mask in a shuffled row order: 10 % masked rows and 5 % NaN labels, and, where the layout
    has three lists of 6 rows or more, the smallest of them with every row masked and the next with all labels equal."""
    sizes = np.asarray(LAYOUTS[layout], dtype=np.int64)
    rng = np.random.default_rng(seed + 17 * len(sizes))
    k = np.repeat(np.arange(sizes.size), sizes)
    B = k.size
    y = _labels(rng, B, labels)
    mask = np.ones(B, np.uint8)
    if B > 1:
        mask[rng.random(B) < 0.10] = 0
        y[rng.random(B) < 0.05] = np.nan
        y[(y == 0) & (rng.random(B) < 0.5)] = -0.0
    small = [g for g in np.argsort(sizes, kind='stable') if sizes[g] >= 6]
    if len(small) >= 3:
        mask[k == small[0]] = 0                       # every row masked
        y[k == small[1]] = 1.0                        # all labels equal
    s = _logits(rng, k, logits)
    p = rng.permutation(B)
    k, y, s, mask = k[p], y[p], s[p], mask[p]
    ids = (k * 3 + 5).astype(np.int64)
    n_members = np.bincount(k, weights=(mask != 0) & ~np.isnan(y), minlength=sizes.size).astype(np.int64)
    for a in (ids, y, s, mask):
        a.setflags(write=False)
    return ids, y, s, mask, _census(sizes, n_members)


@functools.lru_cache(maxsize=None)
def _ref(layout, labels, logits, topn=None, list_mean=False, weighted=False):
    ids, y, s, mask, _ = _case(layout, labels, logits)
    w = None
    if weighted:
        nv = MO.listmle_ref(ids, y, s, mask=mask, topn=topn).n_valid
        w = np.random.default_rng(3).uniform(0.5, 2.0, nv).astype(np.float32)
    return MO.listmle_ref(ids, y, s, weights=w, mask=mask, topn=topn, list_mean=list_mean), w


# ---- running and checking --------------------------------------------------------------------------------------------------------------------
def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _dev_ids(ids, dev):
    return [_t(a, dev) for a in ids] if isinstance(ids, (list, tuple)) else _t(ids, dev)


def _run(dev, ids, y, s, mask=None, weights=None, upstream=None, **kw):
    M = _mod()
    sd = _t(s, dev).requires_grad_(True)
    loss, nv = M.listmle_loss_from_batch(_dev_ids(ids, dev), _t(y, dev), sd, weights=_t(weights, dev), mask=_t(mask, dev), return_num_list=True, **kw)
    if kw.get('do_reduce', True):
        loss.backward()
    elif loss.numel() > 0:
        loss.backward(_t(upstream, dev) if upstream is not None else torch.ones_like(loss))
    grad = sd.grad.cpu().numpy().copy() if sd.grad is not None else np.zeros(s.size, np.float32)
    return loss.detach().cpu().numpy().copy(), int(nv.item()), grad


def _check_grad(name, ref, d, dref):
    d = d.astype(np.float64)
    G = ref.valid.size
    if G == 0:
        return
    assert np.isfinite(d).all(), name
    assert not d[ref.row_rank < 0].any(), '%s: a row of an invalid list has a gradient' % name
    assert not d[ref.position < 0].any(), '%s: a row that does not take part has a gradient' % name
    err, big = np.zeros(G), np.zeros(G)
    np.maximum.at(err, ref.row_list, np.abs(d - dref))
    np.maximum.at(big, ref.row_list, np.abs(dref))
    sums = np.abs(np.bincount(ref.row_list, weights=d, minlength=G))
    v = ref.valid & (big > 0)
    ratio = float((err[v] / (RTOL * big[v])).max()) if v.any() else 0.0
    print('%s: worst per-list gradient error / bound = %.3g, worst per-list |sum| / bound = %.3g' % (
        name, ratio, float((sums[v] / (RTOL * big[v])).max()) if v.any() else 0.0))
    assert (err[ref.valid] <= RTOL * big[ref.valid]).all(), '%s: %d lists beyond their bound, worst ratio %.3g' % (
        name, int((err[ref.valid] > RTOL * big[ref.valid]).sum()), ratio)
    assert (sums[ref.valid] <= RTOL * big[ref.valid]).all(), '%s: a list whose gradient does not sum to zero' % name


def _check_reduced(name, ref, loss, nv, grad):
    print('%s: %d lists, %d valid (kernel %d); loss %.9g ref %.9g' % (name, ref.valid.size, ref.n_valid, nv, float(loss), ref.loss))
    assert nv == ref.n_valid, name
    assert abs(float(loss) - ref.loss) <= RTOL * abs(ref.loss), name
    _check_grad(name, ref, grad, ref.grad)


def _check_terms(name, ref, terms):
    pos, lse = terms.position.cpu().numpy(), terms.lse.cpu().numpy()
    assert np.array_equal(pos, ref.position), name
    assert np.array_equal(terms.valid.cpu().numpy(), ref.valid), name
    m = ref.position >= 0
    assert np.isnan(lse[~m]).all(), name
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.abs(lse[m] - ref.lse[m]) / np.abs(ref.lse[m])
    ratio = np.where(lse[m] == ref.lse[m], 0.0, ratio)
    print('%s: worst |lse - ref| / |ref| = %.3g (bound %.0e)' % (name, float(ratio.max(initial=0.0)), LSE_RTOL))
    assert (ratio <= LSE_RTOL).all(), name
    ll = terms.list_loss.cpu().numpy()
    assert ll.shape == ref.list_loss.shape and (np.abs(ll - ref.list_loss) <= RTOL * np.abs(ref.list_loss)).all(), name


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------------------
def test_the_layouts_reach_every_tile_class():
    c = {name: _case(name)[4] for name in LAYOUTS}
    for key in ('B off the tile', 'more than one tile', 'a list over three tiles', 'a list over two tiles', 'lists of 1, 2 and 3 rows',
                'a tile boundary inside the rows that do not take part', 'a tile boundary inside the members behind place 3', 'a list with no member'):
        assert c['sizes'][key], key
    for key in ('a list begins on a tile boundary', 'a list begins one behind a tile boundary', 'a list over two tiles', 'a list with no member'):
        assert c['boundary'][key], key
    assert c['packed']['a hundred lists in one tile'] and c['packed']['B off the tile'] and c['packed']['more than one tile']
    assert c['one_list']['a list over three tiles'] and not c['single_row']['more than one tile']
    sizes = LAYOUTS['sizes']
    assert all(n in sizes for n in (1, 2, 3, 1023, 1024, 1025, 2049, 3000))
    cum = np.cumsum([0] + sizes)
    assert cum[7] // T + 1 < (cum[8] - 1) // T            # the list of 3000 rows holds a whole tile: its carry crosses one


@pytest.mark.parametrize('layout,labels,logits', [('sizes', 'levels', 'unit'), ('sizes', 'distinct', 'mag120'), ('boundary', 'levels', 'mag120'),
                                                  ('boundary', 'distinct', 'unit'), ('packed', 'levels', 'unit'), ('packed', 'distinct', 'mag120'),
                                                  ('one_list', 'levels', 'unit'), ('one_list', 'distinct', 'mag120'), ('single_row', 'levels', 'unit')])
def test_layout_against_the_oracle(dev, layout, labels, logits):
    name = '%s/%s/%s' % (layout, labels, logits)
    ids, y, s, mask, _ = _case(layout, labels, logits)
    ref, _ = _ref(layout, labels, logits)
    if layout not in ('single_row',):
        assert ref.n_valid >= 1 and (ref.position < 0).any()
    loss, nv, grad = _run(dev, ids, y, s, mask)
    _check_reduced(name, ref, loss, nv, grad)
    loss2, nv2, grad2 = _run(dev, ids, y, s, mask)
    assert loss.tobytes() == loss2.tobytes() and nv == nv2 and grad.tobytes() == grad2.tobytes(), '%s: two runs differ' % name
    M = _mod()
    terms = M.listmle_terms(_t(ids, dev), _t(y, dev), _t(s, dev), mask=_t(mask, dev))
    _check_terms(name, ref, terms)
    terms2 = M.listmle_terms(_t(ids, dev), _t(y, dev), _t(s, dev), mask=_t(mask, dev))
    assert all(torch.equal(a, b) or (a.dtype.is_floating_point and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()) for a, b in zip(terms, terms2))


def test_empty_batch(dev):
    M = _mod()
    z = torch.zeros(0, device=dev)
    s = torch.zeros(0, device=dev, requires_grad=True)
    loss, nv = M.listmle_loss_from_batch(torch.zeros(0, dtype=torch.int64, device=dev), z, s, return_num_list=True)
    loss.backward()
    assert float(loss.detach()) == 0.0 and int(nv.item()) == 0 and s.grad.shape == (0,)
    per = M.listmle_loss_from_batch(torch.zeros(0, dtype=torch.int64, device=dev), z, s, do_reduce=False)
    assert per.shape == (0,)
    terms = M.listmle_terms(torch.zeros(0, dtype=torch.int64, device=dev), z, z)
    assert terms.position.shape == (0,) and terms.lse.shape == (0,) and terms.list_loss.shape == (0,) and terms.valid.shape == (0,)


# ---- options -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['sizes', 'packed'])
@pytest.mark.parametrize('topn,list_mean,weighted', [(1, False, False), (3, True, True), (100000, True, False), (3, False, True)])
def test_topn_list_mean_and_weights(dev, layout, topn, list_mean, weighted):
    name = '%s topn=%s list_mean=%s weighted=%s' % (layout, topn, list_mean, weighted)
    ids, y, s, mask, _ = _case(layout, 'levels', 'unit')
    ref, w = _ref(layout, 'levels', 'unit', topn, list_mean, weighted)
    loss, nv, grad = _run(dev, ids, y, s, mask, weights=w, topn=topn, list_mean=list_mean)
    _check_reduced(name, ref, loss, nv, grad)
    terms = _mod().listmle_terms(_t(ids, dev), _t(y, dev), _t(s, dev), mask=_t(mask, dev), topn=topn)
    _check_terms(name, ref, terms)
    # per list, with an upstream vector
    up = np.random.default_rng(5).normal(size=ref.n_valid).astype(np.float32)
    per, nv, grad = _run(dev, ids, y, s, mask, weights=w, topn=topn, list_mean=list_mean, do_reduce=False, upstream=up)
    assert nv == ref.n_valid and per.shape == (ref.n_valid,)
    assert (np.abs(per - ref.per_list) <= RTOL * np.abs(ref.per_list)).all(), name
    want = ref.dbase * np.where(ref.row_rank >= 0, up.astype(np.float64)[np.maximum(ref.row_rank, 0)], 0.0)
    _check_grad(name + ' per list', ref, grad, want)


def test_weights_of_the_wrong_length_are_refused(dev):
    ids, y, s, mask, _ = _case('packed')
    ref, _ = _ref('packed', 'levels', 'unit')
    with pytest.raises(ValueError, match='one entry per valid list'):
        _run(dev, ids, y, s, mask, weights=np.ones(ref.n_valid - 1, np.float32), do_reduce=False)


def test_logits_as_a_column_of_a_matrix(dev):
    ids, y, s, mask, _ = _case('sizes')
    ref, _ = _ref('sizes', 'levels', 'unit')
    M = _mod()
    x = torch.zeros(s.size, 3, device=dev)
    x[:, 1] = _t(s, dev)
    x.requires_grad_(True)
    loss, nv = M.listmle_loss_from_batch(_t(ids, dev), _t(y, dev).reshape(-1, 1), x[:, 1:2], mask=_t(mask, dev).reshape(-1, 1), return_num_list=True)
    loss.backward()
    g = x.grad.cpu().numpy()
    assert not g[:, 0].any() and not g[:, 2].any()
    _check_reduced('column', ref, loss.detach().cpu().numpy(), int(nv.item()), g[:, 1].copy())


# ---- ids -----------------------------------------------------------------------------------------------------------------------------------------
def test_float_ids_with_special_values_and_two_id_tensors(dev):
    rng = np.random.default_rng(11)
    B = 2600
    y, s = _labels(rng, B, 'levels'), _logits(rng, np.zeros(B, np.int64), 'unit')
    mask = (rng.random(B) < 0.9).astype(np.uint8)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 2.5, -7.0, 1e30], np.float32)
    f = special[rng.integers(0, special.size, B)]                      # -0.0 and +0.0 are one list, equal infinities are one list, every NaN is alone
    ref = MO.listmle_ref(f, y, s, mask=mask)
    assert ref.n_valid >= 5 and (~ref.valid).sum() >= 100
    _check_reduced('float32 ids', ref, *_run(dev, f, y, s, mask))
    _check_terms('float32 ids', ref, _mod().listmle_terms(_t(f, dev), _t(y, dev), _t(s, dev), mask=_t(mask, dev)))
    two = [rng.integers(0, 6, B).astype(np.int64), rng.integers(0, 5, B).astype(np.float32)]
    ref2 = MO.listmle_ref(two, y, s, mask=mask, topn=3)
    assert ref2.n_valid >= 25
    _check_reduced('two id tensors', ref2, *_run(dev, two, y, s, mask, topn=3))
    _check_terms('two id tensors', ref2, _mod().listmle_terms(_dev_ids(two, dev), _t(y, dev), _t(s, dev), mask=_t(mask, dev), topn=3))


# ---- specific cases ------------------------------------------------------------------------------------------------------------------------------
def test_ties_break_by_ascending_row_index(dev):
    """Lists whose labels are all ties but one level apart: the places inside a level follow from the row index alone.  The rows are given in a
    shuffled order, so the place of a row is neither its arrival in the sort nor its position in the list."""
    rng = np.random.default_rng(2)
    sizes = [1500, 40, 9, 1100]
    k = rng.permutation(np.repeat(np.arange(4), sizes))
    B = k.size
    y = (rng.integers(0, 2, B)).astype(np.float32)                      # two levels: ties of hundreds of rows
    s = rng.normal(size=B).astype(np.float32)
    want = np.empty(B, np.int64)
    for g in range(4):
        rows = np.nonzero(k == g)[0]
        hi, lo = rows[y[rows] == 1], rows[y[rows] == 0]                  # ascending row index inside each level
        want[hi] = np.arange(hi.size)
        want[lo] = hi.size + np.arange(lo.size)
    terms = _mod().listmle_terms(_t(k.astype(np.int64), dev), _t(y, dev), _t(s, dev))
    assert np.array_equal(terms.position.cpu().numpy(), want)
    ref = MO.listmle_ref(k, y, s)
    assert np.array_equal(ref.position, want)
    _check_reduced('ties', ref, *_run(dev, k.astype(np.int64), y, s))


def test_non_finite_logits_stay_inside_their_list(dev):
    ids, y, s, mask, _ = _case('sizes')
    ref, _ = _ref('sizes', 'levels', 'unit')
    k = (ids - 5) // 3
    victim = 6                                                          # the list of 2049 rows: it spans tiles, with lists on either side
    rows = np.nonzero((k == victim) & (ref.position >= 0))[0]
    assert ref.valid[ref.row_list[rows[0]]] and rows.size > 1500                 # (the oracle numbers the lists by first occurrence)
    s2 = s.copy()
    s2[rows[np.argsort(ref.position[rows])[[5, 1200]]]] = [np.nan, np.inf]          # places 5 and 1200: in different tiles
    per, nv, grad = _run(dev, ids, y, s, mask, do_reduce=False)
    per2, nv2, grad2 = _run(dev, ids, y, s2, mask, do_reduce=False)
    vr = ref.row_rank[rows[0]]
    others = np.arange(per.size) != vr
    assert nv == nv2 == ref.n_valid
    assert not np.isfinite(per2[vr]) and np.isfinite(per2[others]).all()
    assert per[others].tobytes() == per2[others].tobytes()
    in_list = k == victim
    assert grad[~in_list].tobytes() == grad2[~in_list].tobytes()
    assert np.isnan(grad2[rows]).all() and not grad2[in_list & (ref.position < 0)].any()
    for topn, bad in ((3, -np.inf), (3, np.nan), (None, -np.inf)):      # a non-finite logit behind place K still marks its list, and only it
        s3 = s.copy()
        s3[rows[np.argsort(ref.position[rows])[900]]] = bad
        per0, _, g0 = _run(dev, ids, y, s, mask, do_reduce=False, topn=topn)
        per3, _, g3 = _run(dev, ids, y, s3, mask, do_reduce=False, topn=topn)
        assert not np.isfinite(per3[vr]) and per0[others].tobytes() == per3[others].tobytes() and np.isnan(g3[rows]).all()
        assert g0[~in_list].tobytes() == g3[~in_list].tobytes()


def test_graph_replay_gives_the_eager_bits(dev):
    """Capture and replay of the do_reduce=True call, forward and backward.  The eager step runs on a non-default stream and leaves no reference to
    its autograd graph behind (bench.py --graph has the reason: an AccumulateGrad node made under the legacy default stream and still alive
    makes the end of the capture crash)."""
    ids, y, s, mask, _ = _case('sizes')
    M = _mod()
    gi, yd, md = _t(ids, dev), _t(y, dev), _t(mask, dev)
    sd = _t(s, dev).requires_grad_(True)

    def step():
        loss, nv = M.listmle_loss_from_batch(gi, yd, sd, mask=md, topn=3, list_mean=True, return_num_list=True)
        (g,) = torch.autograd.grad(loss, sd)
        return loss.detach(), nv, g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [o.clone() for o in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = MO.listmle_ref(ids, y, s, mask=mask, topn=3, list_mean=True)
    assert int(eager[1].item()) == ref.n_valid and abs(float(eager[0]) - ref.loss) <= RTOL * abs(ref.loss)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, eager):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_grouping_timeout_poisons_the_loss(dev):
    """RECNOW_DEBUG_GROUP_TIMEOUT=1 makes every barrier of the cooperative grouping launch report a time-out at once (own process: the switch is
    read once).  The inner sort then leaves the identity order and n_seg = -1; the kernels stay in bounds on it and the outputs are poisoned."""
    import subprocess
    import sys
    code = r'''
import numpy as np, torch
from rec_now_amd import _lib
from rec_now_amd.rec_block import listmle
dev = torch.device('cuda:0')
rng = np.random.default_rng(0)
B = 20000
y = torch.from_numpy(rng.integers(0, 3, B).astype(np.float32)).to(dev)
s = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev).requires_grad_(True)
g = torch.from_numpy(rng.integers(0, 20, B).astype(np.int64)).to(dev)
loss, nv = listmle.listmle_loss_from_batch(g, y, s, return_num_list=True)          # both groupings time out
loss.backward()
torch.cuda.synchronize()
assert np.isnan(loss.item()) and nv.item() == -1 and bool(torch.isnan(s.grad).all().item()), (loss, nv)
# segments that are a real grouping, built by hand (20 lists of 1000 rows): only the inner sort times out
P = _lib.ptr
order = torch.from_numpy(np.sort(rng.permutation(B).reshape(20, 1000), axis=1).reshape(-1).astype(np.int32)).to(dev)
seg_id = (torch.arange(B, device=dev) // 1000).to(torch.int32)
seg_first = torch.full((B + 1,), B, dtype=torch.int32, device=dev)
seg_first[:20] = torch.arange(0, B, 1000, dtype=torch.int32, device=dev)
n_seg = torch.tensor([20, 20], dtype=torch.int32, device=dev)
out_loss = torch.zeros((), device=dev)
n_valid = torch.zeros((), dtype=torch.int32, device=dev)
dbase, group_loss = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
ws = _lib.workspace(_lib.load().recnow_listmle_workspace_bytes(B), dev)
for reduce in (0, 1):
    _lib.call('recnow_listmle_fwdbwd', P(y), P(s.detach()), None, None, P(order), P(seg_id), P(seg_first), P(n_seg), B, 3, 1, reduce, P(out_loss), P(n_valid),
              P(dbase), None, P(group_loss), None, None, None, None, P(ws), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    assert np.isnan(out_loss.item()) and n_valid.item() == -1 and bool(torch.isnan(dbase).all().item()) and bool(torch.isnan(group_loss).all().item())
print('poisoned ok')
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=root,
                         env=dict(os.environ, RECNOW_DEBUG_GROUP_TIMEOUT='1', PYTHONPATH=root))
    assert out.returncode == 0 and 'poisoned ok' in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]


def test_c_entry_return_codes(dev):
    from rec_now_amd import _lib
    from rec_now_amd.rec_block._segments import build_segments
    lib = _lib.load()
    P = _lib.ptr
    ids, y, s, mask, _ = _case('packed')
    seg = build_segments(_t(ids, dev), inf_equal=True)
    yd, sd = _t(y, dev), _t(s, dev)
    B = seg.B
    nbytes = lib.recnow_listmle_workspace_bytes(B)
    ws = _lib.workspace(nbytes, dev)
    loss = torch.full((), 7.0, device=dev)
    nv = torch.full((), 7, dtype=torch.int32, device=dev)
    args = lambda n: (P(yd), P(sd), None, None, P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.n_seg), B, 0, 0, 1, P(loss), P(nv), None, None, None,
                      None, None, None, None, P(ws), n, _lib.stream())
    assert lib.recnow_listmle_fwdbwd(*args(nbytes - 1)) == -2                       # RECNOW_EWORKSPACE
    assert lib.recnow_listmle_fwdbwd(*args(nbytes)) == 0                            # every per-row output is optional
    ref = MO.listmle_ref(ids, y, s)
    assert nv.item() == ref.n_valid and abs(loss.item() - ref.loss) <= RTOL * abs(ref.loss)
    assert lib.recnow_listmle_fwdbwd(None, P(sd), *args(nbytes)[2:]) == -1          # RECNOW_EINVAL
    assert lib.recnow_listmle_fwdbwd(*args(nbytes)[:4], None, *args(nbytes)[5:]) == -1
    empty = list(args(nbytes))
    empty[8] = 0
    assert lib.recnow_listmle_fwdbwd(*empty) == 0 and loss.item() == 0.0 and nv.item() == 0

"""GPU: fetch_single_slot, embedding_single_slot, pool_slots and the small helpers of rec_block/embedding_util.py (csrc/slot_fetch.hip) against
the numpy / fp64 oracle of tests/_slot_oracle.py and the reference's own unit-test literals (tests/golden/slot_util.npz).

Copies (fetched ids and weights, masks, embedding rows, pooled ids) must be bit-identical; sums (pooled weights, every gradient) stay within
1e-5 of the output's scale of the fp64 oracle, the project's standing parity bound."""
import itertools

import numpy as np
import pytest
import torch

import _slot_cases
import _slot_oracle as O

pytestmark = pytest.mark.gpu

TARGET = 3
PARITY = 1e-5


def E():
    from rec_now_amd.rec_block import embedding_util
    return embedding_util


def _batch(rng, B, C, sdt, idt, V, n_slots=5, out_of_table=False):
    slots = rng.integers(0, n_slots, (B, C)).astype(sdt)
    lo, hi = (-V // 4, V + V // 4 + 2) if out_of_table else (0, V)
    ids = rng.integers(lo, hi, (B, C)).astype(idt)
    w = rng.normal(size=(B, C)).astype(np.float32)
    return slots, ids, w


def _max_count(slots):
    return int((slots == TARGET).sum(1).max()) if slots.size else 0


def _ncols_modes(slots):
    mc = _max_count(slots)
    return [None, 1, mc, mc + 7]


def _close(got, want, what):
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    err, scale = (np.abs(got - want).max() if got.size else 0.0), max(np.abs(want).max() if want.size else 0.0, 1e-30)
    print('%s: max err %.3g, scale %.3g' % (what, err, scale))
    assert err <= PARITY * scale, '%s: max err %.3g vs scale %.3g' % (what, err, scale)


SHAPES = list(itertools.product([1, 37, 300, 4099], [1, 20, 64, 65, 200]))
DIMS = [1, 8, 16, 30, 70]


# ---- the reference's own cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['table', 'callable'])
def test_reference_fixture_cases(dev, golden, path):
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    get = lambda t: t.detach().cpu().numpy()                                         # noqa: E731
    if path == 'table':
        func = lambda table: E().EmbeddingTable(torch.from_numpy(table).to(dev))     # noqa: E731
    else:
        func = lambda table: (lambda ids, t=torch.from_numpy(table).to(dev): t[ids])      # noqa: E731
    _slot_cases.run_fixture_cases(golden('slot_util'), E(), put, get, func)


# ---- fetch_single_slot -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C', SHAPES)
def test_fetch_single_slot_equals_oracle(dev, B, C):
    rng = np.random.default_rng(B * 1000 + C)
    for sdt, idt in ((np.int32, np.int64), (np.int64, np.int32)):
        slots, ids, w = _batch(rng, B, C, sdt, idt, 1 << 20)
        ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
        for ncols in _ncols_modes(slots):
            for did, dwt in ((0, 0), (-5, 2.5)):
                gi, gw = E().fetch_single_slot(ts, TARGET, ti, tw, default_id=did, default_weight=dwt, ncols=ncols)
                wi, ww = O.fetch_single_slot(slots, TARGET, ids, w, default_id=did, default_weight=dwt, ncols=ncols)
                assert gi.dtype == ti.dtype and gw.dtype == torch.float32
                assert gi.shape == wi.shape and np.array_equal(gi.cpu().numpy(), wi), (sdt, ncols)
                assert np.array_equal(gw.cpu().numpy(), ww), (sdt, ncols)
        gi, gw = E().fetch_single_slot(ts, TARGET, None, tw, ncols=2)
        assert gi is None and np.array_equal(gw.cpu().numpy(), O.fetch_single_slot(slots, TARGET, None, w, ncols=2)[1])
        gi, gw = E().fetch_single_slot(ts, TARGET, ti, None, ncols=2)
        assert gw is None and np.array_equal(gi.cpu().numpy(), O.fetch_single_slot(slots, TARGET, ids, None, ncols=2)[0])
        assert E().fetch_single_slot(ts, TARGET) == (None, None)


def test_slot_absent_from_the_batch(dev):
    rng = np.random.default_rng(5)
    slots, ids, w = _batch(rng, 37, 20, np.int32, np.int64, 100)
    slots[slots == TARGET] = 0
    ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
    gi, gw = E().fetch_single_slot(ts, TARGET, ti, tw)
    assert tuple(gi.shape) == (37, 0) and tuple(gw.shape) == (37, 0)
    table = E().EmbeddingTable(torch.randn(100, 8, device=dev))
    emb, wt, m = E().embedding_single_slot(table, ts, TARGET, ti, tw)
    assert tuple(emb.shape) == (37, 0, 8) and tuple(wt.shape) == (37, 0, 1) and tuple(m.shape) == (37, 0, 1) and m.dtype == torch.bool
    emb.sum().backward()
    assert table.weight.grad is not None and float(table.weight.grad.abs().sum()) == 0.0
    gi, gw = E().fetch_single_slot(ts, TARGET, ti, tw, default_id=9, default_weight=0.5, ncols=3)
    assert bool((gi == 9).all()) and bool((gw == 0.5).all())
    emb, wt, m = E().embedding_single_slot(table, ts, TARGET, ti, tw, ncols=3)
    assert float(emb.detach().abs().sum()) == 0.0 and not bool(m.any())


def test_fetch_weight_gradient(dev):
    rng = np.random.default_rng(9)
    for B, C in ((37, 65), (300, 200), (4099, 20)):
        slots, ids, w = _batch(rng, B, C, np.int32, np.int64, 1000)
        ts, ti = torch.from_numpy(slots).to(dev), torch.from_numpy(ids).to(dev)
        for ncols in _ncols_modes(slots):
            tw = torch.from_numpy(w).to(dev).requires_grad_(True)
            _, gw = E().fetch_single_slot(ts, TARGET, ti, tw, ncols=ncols)
            g = rng.normal(size=tuple(gw.shape)).astype(np.float32)
            gw.backward(torch.from_numpy(g).to(dev))
            _, want = O.embedding_single_slot_grads(1, slots, TARGET, ids, gw.shape[1], np.zeros(tuple(gw.shape) + (1,)), g)
            _close(tw.grad, want, 'd fetch / d weights B=%d C=%d ncols=%s' % (B, C, ncols))


# ---- embedding_single_slot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C', SHAPES)
def test_embedding_single_slot_equals_oracle(dev, B, C):
    rng = np.random.default_rng(B * 77 + C)
    k = SHAPES.index((B, C))
    V = 500
    for n, (sdt, idt) in enumerate(((np.int32, np.int64), (np.int64, np.int32))):
        D = DIMS[(k + n) % len(DIMS)]
        slots, ids, w = _batch(rng, B, C, sdt, idt, V)
        tab = rng.normal(size=(V, D)).astype(np.float32)
        ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
        for ncols in _ncols_modes(slots):
            table = E().EmbeddingTable(torch.from_numpy(tab).to(dev))
            twg = tw.clone().requires_grad_(True)
            emb, wt, m = E().embedding_single_slot(table, ts, TARGET, ti, twg, default_weight=1.5, ncols=ncols)
            we, ww, wm = O.embedding_single_slot(O.table_lookup(tab), slots, TARGET, ids, w, default_weight=1.5, ncols=ncols)
            assert emb.dtype == torch.float32 and m.dtype == torch.bool
            assert emb.shape == we.shape and np.array_equal(emb.detach().cpu().numpy(), we), (D, ncols)        # copies: bit for bit, zero padding
            assert wt.shape == ww.shape and np.array_equal(wt.detach().cpu().numpy(), ww), (D, ncols)
            assert m.shape == wm.shape and np.array_equal(m.cpu().numpy(), wm), (D, ncols)
            ge = rng.normal(size=we.shape).astype(np.float32)
            gw = rng.normal(size=ww.shape).astype(np.float32)
            torch.autograd.backward([emb, wt], [torch.from_numpy(ge).to(dev), torch.from_numpy(gw).to(dev)])
            dt, dw = O.embedding_single_slot_grads(V, slots, TARGET, ids, we.shape[1], ge, gw)
            _close(table.weight.grad, dt, 'd table B=%d C=%d D=%d ncols=%s' % (B, C, D, ncols))
            _close(twg.grad, dw, 'd weights B=%d C=%d D=%d ncols=%s' % (B, C, D, ncols))
        emb, wt, m = E().embedding_single_slot(E().EmbeddingTable(torch.from_numpy(tab).to(dev)), ts, TARGET, ti, None, ncols=2)
        assert wt is None and np.array_equal(emb.detach().cpu().numpy(), O.embedding_single_slot(O.table_lookup(tab), slots, TARGET, ids, ncols=2)[0])


@pytest.mark.parametrize('D', DIMS)
def test_embedding_paths_agree_and_the_callable_sees_sorted_unique_ids(dev, D):
    rng = np.random.default_rng(D)
    B, C, V = 300, 65, 400
    slots, ids, w = _batch(rng, B, C, np.int32, np.int64, V)
    tab = torch.from_numpy(rng.normal(size=(V, D)).astype(np.float32)).to(dev)
    ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
    ncols = _max_count(slots) - 2
    g = torch.from_numpy(rng.normal(size=(B, ncols, D)).astype(np.float32)).to(dev)
    results = {}
    for path in ('table', 'callable_unique', 'callable_no_unique'):
        param = torch.nn.Parameter(tab.clone())
        seen = []

        def lookup(q, param=param, seen=seen):
            seen.append(q.detach().cpu().numpy())
            return param[q]
        func = E().EmbeddingTable(param) if path == 'table' else lookup
        emb, wt, m = E().embedding_single_slot(func, ts, TARGET, ti, tw, ncols=ncols, use_unique=path != 'callable_no_unique')
        emb.backward(g)
        results[path] = (emb.detach(), wt.detach(), m, param.grad.clone())
        sel = ids[slots == TARGET]
        if path == 'callable_unique':
            assert len(seen) == 1 and seen[0].dtype == np.int64 and np.array_equal(seen[0], np.unique(sel))
        if path == 'callable_no_unique':
            assert len(seen) == 1 and np.array_equal(seen[0], sel)
    dt, _ = O.embedding_single_slot_grads(V, slots, TARGET, ids, ncols, g.cpu().numpy())
    for path in ('callable_unique', 'callable_no_unique'):
        for a, b in zip(results['table'][:3], results[path][:3]):
            assert torch.equal(a, b), path
        _close(results[path][3], dt, 'd table through %s, D=%d' % (path, D))
    _close(results['table'][3], dt, 'd table, D=%d' % D)


@pytest.mark.parametrize('sparse', [False, True])
def test_table_gradient_is_bit_identical_from_run_to_run(dev, sparse):
    rng = np.random.default_rng(21)
    B, C, V, D = 4099, 64, 50, 16                      # few ids: long segments, chunk joins
    slots, ids, w = _batch(rng, B, C, np.int32, np.int64, V)
    ts, ti = torch.from_numpy(slots).to(dev), torch.from_numpy(ids).to(dev)
    ncols = _max_count(slots)
    g = torch.from_numpy(rng.normal(size=(B, ncols, D)).astype(np.float32)).to(dev)
    grads = []
    for _ in range(2):
        table = E().EmbeddingTable(torch.ones(V, D, device=dev), sparse_grad=sparse)
        emb, _, _ = E().embedding_single_slot(table, ts, TARGET, ti, ncols=ncols)
        emb.backward(g)
        gr = table.weight.grad
        assert gr.is_sparse == sparse
        grads.append(gr.to_dense() if sparse else gr.clone())
    assert torch.equal(grads[0], grads[1])
    dt, _ = O.embedding_single_slot_grads(V, slots, TARGET, ids, ncols, g.cpu().numpy())
    _close(grads[0], dt, 'd table (sparse_grad=%s)' % sparse)


@pytest.mark.parametrize('sparse', [False, True])
def test_ids_outside_the_table(dev, sparse):
    rng = np.random.default_rng(31)
    B, C, V, D = 300, 64, 40, 8
    slots, ids, w = _batch(rng, B, C, np.int64, np.int64, V, out_of_table=True)
    assert ((ids < 0) & (slots == TARGET)).any() and ((ids >= V) & (slots == TARGET)).any()
    tab = rng.normal(size=(V, D)).astype(np.float32)
    table = E().EmbeddingTable(torch.from_numpy(tab).to(dev), sparse_grad=sparse)
    ncols = _max_count(slots)
    emb, _, m = E().embedding_single_slot(table, torch.from_numpy(slots).to(dev), TARGET, torch.from_numpy(ids).to(dev), ncols=ncols)
    we, _, wm = O.embedding_single_slot(O.table_lookup(tab), slots, TARGET, ids, ncols=ncols)
    assert np.array_equal(emb.detach().cpu().numpy(), we) and np.array_equal(m.cpu().numpy(), wm)
    fetched, _ = O.fetch_single_slot(slots, TARGET, ids, default_id=0, ncols=ncols)
    outside = ((fetched < 0) | (fetched >= V)) & wm[..., 0]
    assert outside.any() and float(np.abs(emb.detach().cpu().numpy()[outside]).sum()) == 0.0        # zero rows, mask True
    g = rng.normal(size=we.shape).astype(np.float32)
    emb.backward(torch.from_numpy(g).to(dev))
    gr = table.weight.grad
    if sparse:
        idx = gr.coalesce().indices()
        assert int(idx.min()) >= 0 and int(idx.max()) < V
        gr = gr.to_dense()
    assert tuple(gr.shape) == (V, D)
    _close(gr, O.embedding_single_slot_grads(V, slots, TARGET, ids, ncols, g)[0], 'd table with ids outside the table (sparse_grad=%s)' % sparse)


# ---- pool_slots --------------------------------------------------------------------------------------------------------------------------------
def _pool_batch(rng, B, C, sdt, idt):
    """Slots drawn from few values in runs: equal adjacent and equal non-adjacent slots both occur in most rows."""
    slots = rng.integers(0, 6, (B, C))
    rep = rng.random((B, C)) < 0.4
    for c in range(1, C):
        slots[:, c] = np.where(rep[:, c], slots[:, c - 1], slots[:, c])
    ids = rng.integers(0, np.iinfo(idt).max, (B, C), dtype=np.int64).astype(idt)
    return slots.astype(sdt), ids, rng.normal(size=(B, C)).astype(np.float32)


@pytest.mark.parametrize('B,C', SHAPES)
def test_pool_slots_equals_oracle(dev, B, C):
    rng = np.random.default_rng(B * 13 + C)
    targets = [4, 1, 9, 2]                             # 9 never occurs: an empty segment in every row
    for sdt, idt in ((np.int32, np.int64), (np.int64, np.int32)):
        slots, ids, w = _pool_batch(rng, B, C, sdt, idt)
        if C >= 20:                                    # the literal rule differs from a full dedupe on this batch, in both directions
            seg = O.batch_segment_ids_of_targets(slots, targets)[0]
            literal = O.first_occurance_in_row(seg, False, -1) >= 0
            first = np.zeros_like(literal)
            for r, row in enumerate(seg):
                _, where = np.unique(row, return_index=True)
                first[r, where] = True
            first &= seg >= 0
            assert ((seg >= 0) & ~literal).any() and (literal & ~first).any()
        ts, ti = torch.from_numpy(slots).to(dev), torch.from_numpy(ids).to(dev)
        for method, drop in itertools.product(('sum', 'mean'), (False, True)):
            tw = torch.from_numpy(w).to(dev).requires_grad_(True)
            pi, pw = E().pool_slots(ts, targets, ti, tw, method=method, drop_duplicate_slot=drop)
            wi, ww = O.pool_slots(slots, targets, ids, w.astype(np.float64), method=method, drop_duplicate_slot=drop)
            assert pi.dtype == ti.dtype and tuple(pi.shape) == (B, 4) and np.array_equal(pi.cpu().numpy(), wi), (method, drop)
            _close(pw, ww, 'pooled_weights %s drop=%s B=%d C=%d' % (method, drop, B, C))
            g = rng.normal(size=(B, 4)).astype(np.float32)
            pw.backward(torch.from_numpy(g).to(dev))
            _close(tw.grad, O.pool_slots_weight_grad(slots, targets, method, drop, g), 'd pooled_weights / d weights %s drop=%s' % (method, drop))
        pi, pw = E().pool_slots(ts, targets, ti)
        assert pw is None and np.array_equal(pi.cpu().numpy(), O.pool_slots(slots, targets, ids)[0])
        pi, pw = E().pool_slots(ts, targets, None, torch.from_numpy(w).to(dev))
        assert pi is None
        _close(pw, O.pool_slots(slots, targets, None, w.astype(np.float64))[1], 'pooled_weights without ids')


def test_pool_slots_dtype_max_many_targets_and_one_row(dev):
    for idt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        big = np.iinfo(idt).max
        slots = np.array([[2, 0, 5, 5], [5, 2, 2, 0]], dtype=np.int32)
        ids = np.array([[big, 1, 7, 3], [big, big, 4, 1]], dtype=idt)
        pi, _ = E().pool_slots(torch.from_numpy(slots).to(dev), [2, 5, 8], torch.from_numpy(ids).to(dev))
        assert pi.dtype == tdt and pi.cpu().tolist() == [[0, 3, 0], [4, 0, 0]]
        assert np.array_equal(pi.cpu().numpy(), O.pool_slots(slots, [2, 5, 8], ids)[0])
    rng = np.random.default_rng(3)
    T = 150                                             # more targets than lanes: three target groups per row
    slots = rng.integers(0, 200, (37, 300)).astype(np.int64)
    ids = rng.integers(0, 1 << 40, (37, 300))
    w = rng.normal(size=(37, 300)).astype(np.float32)
    targets = [int(t) for t in rng.permutation(200)[:T]]
    pi, pw = E().pool_slots(torch.from_numpy(slots).to(dev), targets, torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev), method='mean')
    wi, ww = O.pool_slots(slots, targets, ids, w.astype(np.float64), method='mean')
    assert np.array_equal(pi.cpu().numpy(), wi)
    _close(pw, ww, 'pooled_weights, 150 targets')
    pi, pw = E().pool_slots(torch.from_numpy(slots[0]).to(dev), targets, torch.from_numpy(ids[0]).to(dev), torch.from_numpy(w[0]).to(dev))
    assert tuple(pi.shape) == (1, T) and np.array_equal(pi.cpu().numpy(), O.pool_slots(slots[0], targets, ids[:1])[0])
    _close(pw, O.pool_slots(slots[0], targets, None, w[:1].astype(np.float64))[1], 'pooled_weights of 1-D slots')


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------
def test_small_helpers_equal_oracle(dev):
    rng = np.random.default_rng(17)
    E_ = E()
    for dt in (np.int32, np.int64):
        v = rng.integers(0, 12, (37, 65)).astype(dt)
        tv = torch.from_numpy(v).to(dev)
        assert np.array_equal(E_.isin(tv, [3, 5, 5, 11]).cpu().numpy(), O.isin(v, [3, 5, 11]))
        assert np.array_equal(E_.isin(tv.reshape(-1), [3]).cpu().numpy(), O.isin(v.reshape(-1), [3]))
        mv = E_.mask_values(tv, [3, 5, 11], padding_value=-2)
        assert mv.dtype == tv.dtype and np.array_equal(mv.cpu().numpy(), O.mask_values(v, [3, 5, 11], -2))
        for need_sort in (False, True):
            got = E_.first_occurance_in_row(tv, need_sort=need_sort, padding_value=-1)
            assert np.array_equal(got.cpu().numpy(), O.first_occurance_in_row(v, need_sort, -1))
        seg, nr, ni, ns = E_.batch_segment_ids_of_targets(tv, [5, 3, 0])
        ws, wr, wi, wn = O.batch_segment_ids_of_targets(v, [5, 3, 0])
        assert np.array_equal(seg.cpu().numpy(), ws) and (nr, ni, ns) == (wr, wi, wn)
        with pytest.warns(UserWarning):
            si, sw = E_.pool_single_slot(tv, 3, tv * 10, tv.float())
        wi, ww = O.pool_single_slot(v, 3, v * 10, v.astype(np.float32))
        assert np.array_equal(si.cpu().numpy(), wi) and np.array_equal(sw.cpu().numpy(), ww)


def test_old_pooled_lookups_route_to_the_fused_one(dev):
    rng = np.random.default_rng(2)
    slots, ids, w = _batch(rng, 37, 20, np.int32, np.int64, 60)
    ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
    table = E().EmbeddingTable(torch.randn(60, 8, device=dev))
    want = E().embedding_using_sparse_batch_segment_ids(table, ts, [1, 3], ti, tw)
    assert torch.equal(E().embedding_using_batch_segment_ids(table, ts, [1, 3], ti, tw), want)
    assert torch.equal(E().embedding_using_sparse_batch_segment_ids_v1(table, ts, [1, 3], ti, weights=tw), want)


# ---- every element written, nothing beyond -----------------------------------------------------------------------------------------------------
def test_kernels_write_every_output_element_and_nothing_beyond(dev):
    """Through the C ABI: each output is the head of a larger buffer prefilled with a sentinel (NaN / -999 / 0x5a) no kernel writes."""
    from rec_now_amd import _lib
    rng = np.random.default_rng(41)
    B, C, D, V, T, TAIL = 37, 65, 30, 90, 3, 1000
    slots, ids, w = _batch(rng, B, C, np.int32, np.int64, V)
    ts, ti, tw = (torch.from_numpy(a).to(dev) for a in (slots, ids, w))
    tab = torch.randn(V, D, device=dev)
    for ncols in (1, _max_count(slots) + 7):
        n = B * ncols
        f = lambda k: torch.full((k + TAIL,), float('nan'), device=dev)              # noqa: E731
        o_ids = torch.full((n + TAIL,), -999, dtype=torch.int64, device=dev)
        o_w, o_e, o_w2 = f(n), f(n * D), f(n)
        o_m, o_m2 = (torch.full((n + TAIL,), 0x5a, dtype=torch.uint8, device=dev) for _ in range(2))
        o_src, o_src2, o_k32 = (torch.full((n + TAIL,), -999, dtype=torch.int32, device=dev) for _ in range(3))
        o_key = torch.full((n + TAIL,), -999, dtype=torch.int64, device=dev)
        _lib.call('recnow_slot_fetch', _lib.ptr(ts), 2, TARGET, _lib.ptr(ti), 3, _lib.ptr(tw), B, C, ncols, -777, 0.25, _lib.ptr(o_ids),
                  _lib.ptr(o_w), _lib.ptr(o_m), _lib.ptr(o_src), _lib.stream())
        _lib.call('recnow_slot_embed_fwd', _lib.ptr(tab), D, V, _lib.ptr(ts), 2, TARGET, _lib.ptr(ti), 3, _lib.ptr(tw), B, C, ncols, 0.25,
                  _lib.ptr(o_e), _lib.ptr(o_w2), _lib.ptr(o_m2), _lib.ptr(o_src2), _lib.ptr(o_key), _lib.ptr(o_k32), V, _lib.stream())
        torch.cuda.synchronize()
        wi, ww = O.fetch_single_slot(slots, TARGET, ids, w, default_id=-777, default_weight=0.25, ncols=ncols)
        we, _, wm = O.embedding_single_slot(O.table_lookup(tab.cpu().numpy()), slots, TARGET, ids, ncols=ncols)
        src = O.positions(slots, TARGET, ncols)
        assert np.array_equal(o_ids[:n].cpu().numpy().reshape(B, ncols), wi) and bool((o_ids[n:] == -999).all())
        assert np.array_equal(o_w[:n].cpu().numpy().reshape(B, ncols), ww) and bool(torch.isnan(o_w[n:]).all())
        assert np.array_equal(o_e[:n * D].cpu().numpy().reshape(B, ncols, D), we) and bool(torch.isnan(o_e[n * D:]).all())
        assert np.array_equal(o_w2[:n].cpu().numpy().reshape(B, ncols), ww) and bool(torch.isnan(o_w2[n:]).all())
        for m in (o_m, o_m2):
            assert np.array_equal(m[:n].cpu().numpy().reshape(B, ncols, 1), wm.astype(np.uint8)) and bool((m[n:] == 0x5a).all())
        for s in (o_src, o_src2):
            assert np.array_equal(s[:n].cpu().numpy().reshape(B, ncols), src) and bool((s[n:] == -999).all())
        key = np.where(src >= 0, wi, V)
        assert np.array_equal(o_key[:n].cpu().numpy().reshape(B, ncols), key) and bool((o_key[n:] == -999).all())
        assert np.array_equal(o_k32[:n].cpu().numpy().reshape(B, ncols), key) and bool((o_k32[n:] == -999).all())
        # fetch backward: (B, C) written in full
        dw = torch.full((B * C + TAIL,), float('nan'), device=dev)
        g = torch.randn(n, device=dev)
        _lib.call('recnow_slot_fetch_bwd', _lib.ptr(o_src), _lib.ptr(g), B, C, ncols, _lib.ptr(dw), _lib.stream())
        torch.cuda.synchronize()
        want = O.embedding_single_slot_grads(1, slots, TARGET, ids, ncols, np.zeros((B, ncols, 1)), g.cpu().numpy().reshape(B, ncols))[1]
        assert np.array_equal(dw[:B * C].cpu().numpy().reshape(B, C), want.astype(np.float32)) and bool(torch.isnan(dw[B * C:]).all())
    # pool_slots
    index = {1: 0, TARGET: 1, 4: 2}
    seg = torch.from_numpy(np.array([[index.get(int(v), -1) for v in row] for row in slots], dtype=np.int32)).to(dev)
    p_ids = torch.full((B * T + TAIL,), -999, dtype=torch.int64, device=dev)
    p_w, p_c, p_dw = (torch.full((k + TAIL,), float('nan'), device=dev) for k in (B * T, B * T, B * C))
    _lib.call('recnow_slot_pool_fwd', _lib.ptr(seg), _lib.ptr(ti), 3, _lib.ptr(tw), B, C, T, 1, 1, _lib.ptr(p_ids), _lib.ptr(p_w), _lib.ptr(p_c), _lib.stream())
    g = torch.randn(B * T, device=dev)
    _lib.call('recnow_slot_pool_bwd', _lib.ptr(seg), _lib.ptr(p_c), _lib.ptr(g), B, C, T, 1, 1, _lib.ptr(p_dw), _lib.stream())
    torch.cuda.synchronize()
    wi, ww = O.pool_slots(slots, [1, TARGET, 4], ids, w.astype(np.float64), method='mean', drop_duplicate_slot=True)
    assert np.array_equal(p_ids[:B * T].cpu().numpy().reshape(B, T), wi) and bool((p_ids[B * T:] == -999).all())
    _close(p_w[:B * T].reshape(B, T), ww, 'pooled_weights in a sentinel buffer')
    for buf, k in ((p_w, B * T), (p_c, B * T), (p_dw, B * C)):
        assert not bool(torch.isnan(buf[:k]).any()) and bool(torch.isnan(buf[k:]).all())


# ---- composition and graph capture -------------------------------------------------------------------------------------------------------------
def test_sequence_embedding_into_dot_product_attention(dev):
    import dense_ref as R
    from rec_now_amd.rec_block.attention import attention_by_dot_product
    rng = np.random.default_rng(51)
    B, C, V, D, ncols = 300, 65, 200, 16, 12
    slots, ids, _ = _batch(rng, B, C, np.int32, np.int64, V)
    tab = rng.normal(0, 0.3, (V, D)).astype(np.float32)
    doc = rng.normal(0, 0.3, (B, D)).astype(np.float32)
    table = E().EmbeddingTable(torch.from_numpy(tab).to(dev))
    emb, _, _ = E().embedding_single_slot(table, torch.from_numpy(slots).to(dev), TARGET, torch.from_numpy(ids).to(dev), ncols=ncols)
    mat, ssum = attention_by_dot_product(emb, torch.from_numpy(doc).to(dev))
    loss = mat.sum() + ssum.sum()
    loss.backward()
    t64 = torch.from_numpy(tab).double().requires_grad_(True)
    src = O.positions(slots, TARGET, ncols)
    rows = np.where(src >= 0, np.take_along_axis(ids, np.maximum(src, 0), 1), 0)
    e64 = t64[torch.from_numpy(rows)] * torch.from_numpy(src >= 0).double()[..., None]
    assert np.array_equal(e64.detach().numpy().astype(np.float32), O.embedding_single_slot(O.table_lookup(tab), slots, TARGET, ids, ncols=ncols)[0])
    rm, rs = R.attention_by_dot_product(e64, torch.from_numpy(doc).double())
    ref = rm.sum() + rs.sum()
    ref.backward()
    _close(loss.reshape(1), ref.detach().numpy().reshape(1), 'loss of embedding_single_slot -> attention_by_dot_product')
    _close(table.weight.grad, t64.grad.numpy(), 'd loss / d table')


def test_forward_with_explicit_ncols_is_graph_capturable(dev):
    """No hidden sync, no host-side size: the three fused forwards are captured once and replayed on new input contents."""
    rng = np.random.default_rng(61)
    B, C, V, D, ncols = 300, 65, 200, 8, 9
    targets = [1, TARGET, 4]
    a, b = _batch(rng, B, C, np.int32, np.int64, V), _batch(rng, B, C, np.int32, np.int64, V)
    ts, ti, tw = (torch.from_numpy(x).to(dev) for x in a)
    table = E().EmbeddingTable(torch.randn(V, D, device=dev))

    def step():
        with torch.no_grad():
            fi, fw = E().fetch_single_slot(ts, TARGET, ti, tw, default_id=-1, default_weight=0.5, ncols=ncols)
            emb, wt, m = E().embedding_single_slot(table, ts, TARGET, ti, tw, ncols=ncols)
            pi, pw = E().pool_slots(ts, targets, ti, tw, method='mean', drop_duplicate_slot=True)
        return fi, fw, emb, wt, m, pi, pw
    step()                                              # the (cached) upload of the target list happens outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for x, y in zip((ts, ti, tw), b):                   # new contents, same storage
        x.copy_(torch.from_numpy(y).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    want = step()
    torch.cuda.synchronize()
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    assert np.array_equal(got[0].cpu().numpy(), O.fetch_single_slot(b[0], TARGET, b[1], default_id=-1, ncols=ncols)[0])

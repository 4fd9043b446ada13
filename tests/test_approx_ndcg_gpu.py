"""In-batch ApproxNDCG (rec_block/approx_ndcg.py, csrc/pairwise_approx.hip) against the list-by-list fp64 oracle tests/_approx_ndcg_oracle.py
(pinned on the CPU in tests/test_approx_ndcg_cpu.py).

Routes.  The three layouts of tests/_pair_lists_oracle.py (3513 to 6425 rows) reach, between them, every class of O.CLASSES;
`test_every_route_class_is_reached` reads `seg_first` back and asserts it.  Each layout runs with and without the mask at both temperatures,
once with one group tensor and the exp2 gain, once with two group tensors and the linear gain.

Bounds.  n_lists and the validity of every segment exact; approx_rank within 1e-6 (2 + R) for every taking-part row (the project's 1e-6 bound on
discounts, applied to the quantity the discount is taken of); list_idcg and list_adcg within 1e-6 relative; the loss within 1e-5; the
gradient within 1e-5 of EACH valid list's own largest entry, no list left out; rows of invalid lists and rows that do not take part exactly 0;
each list's gradient sum within 4 n 2**-24 of its largest entry (the pair terms cancel exactly because sigma' is bit-symmetric: only the
float32 rounding of each stored entry remains).  Every case prints its worst ratio to each bound before it asserts."""
import os

import numpy as np
import pytest
import torch

import _approx_ndcg_oracle as AO
import _pair_lists_oracle as O

pytestmark = pytest.mark.gpu
NAMES = tuple(O.LAYOUTS)
EINVAL, EWORKSPACE = -1, -2
NAN = float('nan')


def _mod():
    from rec_now_amd.rec_block import approx_ndcg as M
    return M


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)         # a copy: the shared layouts and references stay as they are


def _groups(name, variant):
    g = O.layout(name)[0]
    return [g, O.second_groups(g.size)] if variant == 'two' else g


def _dev_groups(g, dev):
    return [_t(t, dev) for t in g] if isinstance(g, list) else _t(g, dev)


_REF = {}


def _ref(name, variant, use_mask, gain, tau):
    key = (name, variant, use_mask, gain, tau)
    if key not in _REF:
        _, s, y, mask = O.layout(name)
        _REF[key] = AO.approx_ndcg(s, y, _groups(name, variant), mask if use_mask else None, gain, tau)
    return _REF[key]


def _segments(groups_dev):
    from rec_now_amd.rec_block._segments import build_segments
    return build_segments(groups_dev)


def _lists_of_segments(seg, ref):
    """for every segment of the library the oracle's list it is (a segment IS a list: the same rows); every list appears once"""
    B = seg.B
    order = seg.order.cpu().numpy()
    sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), B)
    n_seg = sf.size - 1
    assert n_seg == len(ref.lists) == seg.num_segments()
    lid = np.empty(n_seg, dtype=np.int64)
    for k in range(n_seg):
        rows = np.sort(order[sf[k]:sf[k + 1]])
        lid[k] = ref.list_id[rows[0]]
        assert np.array_equal(rows, ref.lists[lid[k]])
    assert np.unique(lid).size == n_seg
    return lid


def _run(dev, s, y, groups, mask, gain, tau, segments=None, upstream=None):
    """(loss, n_lists, grad) as numpy / python values"""
    M = _mod()
    sd = _t(np.asarray(s, dtype=np.float32), dev).requires_grad_(True)
    loss, n = M.approx_ndcg_loss(sd, _t(np.asarray(y, dtype=np.float32), dev), None if groups is None else _dev_groups(groups, dev),
                                 None if mask is None else _t(mask, dev), gain, tau, segments=segments, return_num_list=True)
    assert loss.dtype == torch.float32 and loss.shape == () and n.shape == ()
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach().cpu().numpy().copy(), float(n.item()), sd.grad.cpu().numpy().copy()


def _check(dev, s, y, groups, mask, gain, tau, ref, what):
    """every bound of the module docstring, list by list; returns the worst ratios"""
    M = _mod()
    s, y = np.asarray(s, dtype=np.float32), np.asarray(y, dtype=np.float32)
    B = s.size
    take = np.ones(B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    gd = _dev_groups(groups, dev)
    seg = _segments(gd)
    lid = _lists_of_segments(seg, ref)
    terms = M.approx_ndcg_terms(_t(s, dev), _t(y, dev), None, None if mask is None else _t(mask, dev), gain, tau, segments=seg)
    assert [t.dtype for t in terms] == [torch.float64] * 4 + [torch.int64] and terms.approx_rank.shape == (B,)
    loss, n, grad = _run(dev, s, y, groups, mask, gain, tau)
    R, adcg, idcg = (t.cpu().numpy() for t in terms[:3])
    adcg, idcg = adcg[:lid.size], idcg[:lid.size]
    worst = {}
    # exact: the number of lists, the validity of every segment, NaN positions, zeros
    assert n == ref.n_lists == terms.n_lists.item()
    assert np.array_equal(idcg > 0, ref.valid[lid])
    assert np.isnan(R[~take]).all() and not np.isnan(R[take]).any()
    dead = ~take | ~ref.valid[ref.list_id]
    assert (grad[dead] == 0).all()
    worst['rank'] = float((np.abs(R[take] - ref.approx_rank[take]) / (1e-6 * (2.0 + ref.approx_rank[take]))).max()) if take.any() else 0.0
    for name, got, want in (('idcg', idcg, ref.idcg[lid]), ('adcg', adcg, ref.adcg[lid])):
        nz = want != 0
        assert (got[~nz] == 0).all()
        worst[name] = float((np.abs(got[nz] - want[nz]) / (1e-6 * np.abs(want[nz]))).max()) if nz.any() else 0.0
    worst['loss'] = abs(float(loss) - ref.loss) / 1e-5
    worst['loss_sum'] = abs(terms.loss_sum.item() - ref.loss_sum) / (1e-6 * max(abs(ref.loss_sum), 1e-300))
    worst['grad'], worst['sum'] = 0.0, 0.0
    for g, rows in enumerate(ref.lists):
        if not ref.valid[g]:
            continue
        top = np.abs(ref.grad[rows]).max()
        nt = int(take[rows].sum())
        if top == 0:
            assert (grad[rows] == 0).all()
            continue
        worst['grad'] = max(worst['grad'], float(np.abs(grad[rows] - ref.grad[rows]).max() / (1e-5 * top)))
        worst['sum'] = max(worst['sum'], abs(float(grad[rows].astype(np.float64).sum())) / (4 * nt * 2.0 ** -24 * float(np.abs(grad[rows]).max())))
    print('approx_ndcg %s: worst ratio to its bound: %s' % (what, ', '.join('%s %.3g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= 1.0, '%s: %s exceeds its bound by a factor of %.3g' % (what, k, v)
    return worst


def _terms(dev, s, y, groups, mask, tau):
    """the five outputs of approx_ndcg_terms as numpy, the per-list ones cut to the segments that exist (the entries behind them are not written)"""
    gd = _dev_groups(groups, dev)
    n_seg = _segments(gd).num_segments()
    t = _mod().approx_ndcg_terms(_t(s, dev), _t(y, dev), gd, None if mask is None else _t(mask, dev), 'exp2', tau)
    return [t.approx_rank.cpu().numpy(), t.list_adcg.cpu().numpy()[:n_seg], t.list_idcg.cpu().numpy()[:n_seg], t.loss_sum.cpu().numpy(),
            t.n_lists.cpu().numpy()]


# ---- every route ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant,gain', [('one', 'exp2'), ('two', 'linear')])
@pytest.mark.parametrize('tau', [0.1, 1.0])
@pytest.mark.parametrize('use_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('name', NAMES)
def test_layout_list_by_list(dev, name, use_mask, tau, variant, gain):
    ref = _ref(name, variant, use_mask, gain, tau)
    _, s, y, mask = O.layout(name)
    _check(dev, s, y, _groups(name, variant), mask if use_mask else None, gain, tau, ref,
           '%s %s tau=%g %s %s' % (name, 'mask' if use_mask else 'nomask', tau, variant, gain))


def test_every_route_class_is_reached(dev):
    """From the segments the library itself builds: the sizes in sorted order are the layout's, and every class of routes is non-empty in at
    least one layout."""
    got = {}
    for name in NAMES:
        g = O.layout(name)[0]
        seg = _segments(_t(g, dev))
        assert seg.B == g.size
        sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), seg.B)
        assert np.diff(sf).tolist() == O.LAYOUTS[name] and sf.size - 1 == seg.num_segments()
        got[name] = O.census(seg.seg_first.cpu().numpy(), seg.B)
    for cls in O.CLASSES:
        assert any(c[cls] > 0 for c in got.values()), 'no layout reaches %s' % cls
    assert got['r2049']['t_range_2049'] and got['r2049']['t_global'] and got['r2048']['t_range_2048'] and got['r2048']['t_global']


def _masked_list_case():
    """the layout r2049 with its mask, and every row of the list of 37 masked out as well"""
    groups, s, y, mask = O.layout('r2049')
    m = np.array(mask)
    m[groups == 2] = False
    return groups, s, y, m


def test_the_cases_are_telling():
    """From the oracle alone: between the cases there is a list with IDCG = 0, a list of one row, a list with tied scores and a list where
    every row is masked out."""
    ref = _ref('r2048', 'one', True, 'exp2', 0.1)
    assert (~ref.valid).any() and ref.n_lists == 10 and len(ref.lists) == 11
    for name in ('r2049', 'chain'):
        assert _ref(name, 'one', True, 'exp2', 0.1).valid.all()
    assert any(rows.size == 1 for rows in ref.lists)
    s = O.layout('r2048')[1]
    assert any(np.unique(s[rows]).size < rows.size for rows in ref.lists)
    groups, s, y, m = _masked_list_case()
    assert (groups == 2).sum() == 37 and not m[groups == 2].any()


def test_a_list_with_every_row_masked_out(dev):
    groups, s, y, m = _masked_list_case()
    for tau in (0.1, 1.0):
        ref = AO.approx_ndcg(s, y, groups, m, 'exp2', tau)
        assert ref.n_lists == 11 and (ref.idcg == 0).sum() == 1
        _check(dev, s, y, groups, m, 'exp2', tau, ref, 'r2049 with the list of 37 masked out, tau=%g' % tau)


# ---- hand cases -----------------------------------------------------------------------------------------------------------------------------
def test_empty_batch_and_single_row(dev):
    M = _mod()
    e = torch.zeros(0, device=dev)
    s0 = e.clone().requires_grad_(True)
    loss, n = M.approx_ndcg_loss(s0, e, e, return_num_list=True)
    loss.backward()
    assert loss.item() == 0.0 and n.item() == 0.0 and s0.grad.shape == (0,)
    t = M.approx_ndcg_terms(e, e, e)
    assert t.approx_rank.shape == (0,) and t.loss_sum.item() == 0.0 and t.n_lists.item() == 0
    for label, want, n_want in ((2.0, -1.0, 1), (0.0, 0.0, 0)):           # one row: R = 0, ADCG = IDCG = G; invalid with gain 0
        loss, n, grad = _run(dev, [0.3], [label], np.zeros(1, dtype=np.float32), None, 'exp2', 0.1)
        assert float(loss) == want and n == n_want and grad.tolist() == [0.0]
    t = M.approx_ndcg_terms(torch.tensor([0.3], device=dev), torch.tensor([2.0], device=dev), torch.zeros(1, device=dev))
    assert t.approx_rank.tolist() == [0.0] and t.list_idcg.tolist() == [3.0]
    assert abs(t.list_adcg.item() - 3.0) <= 1e-12 and abs(t.loss_sum.item() + 1.0) <= 1e-12


@pytest.mark.parametrize('tau', [0.1, 1.0])
def test_hand_cases(dev, tau):
    g = np.zeros(2, dtype=np.float32)
    # a list of 2
    for s, y in (([0.25, -0.5], [0.0, 1.0]), ([1.0, 1.0], [3.0, 1.0]), ([-2.0, 0.125], [2.0, 2.0])):
        ref = AO.approx_ndcg(s, y, g, None, 'exp2', tau)
        _check(dev, s, y, g, None, 'exp2', tau, ref, 'list of 2 %s %s tau=%g' % (s, y, tau))
    # all labels 0: no valid list, loss 0, gradient 0
    groups, s, _, mask = O.layout('r2049')
    loss, n, grad = _run(dev, s, np.zeros_like(s), groups, mask, 'exp2', tau)
    assert float(loss) == 0.0 and n == 0 and (grad == 0).all()
    # equal scores throughout: every R_i = (n - 1) / 2, and the gradient follows from c alone
    rng = np.random.default_rng(9)
    sizes = [1, 2, 65, 600, 300]
    groups = np.repeat(np.arange(len(sizes)), sizes).astype(np.float32)
    rng.shuffle(groups)
    y = rng.integers(0, 4, groups.size).astype(np.float32)
    s = np.full(groups.size, 0.375, dtype=np.float32)
    ref = AO.approx_ndcg(s, y, groups, None, 'linear', tau)
    for rows in ref.lists:
        assert np.abs(ref.approx_rank[rows] - (rows.size - 1) / 2).max() <= 1e-12 * rows.size
    _check(dev, s, y, groups, None, 'linear', tau, ref, 'equal scores tau=%g' % tau)


def test_small_temperature_against_in_batch_ndcg(dev):
    from rec_now_amd.rec_block.ndcg import in_batch_ndcg
    groups, s, y = AO.tie_free_batch([1, 2, 3, 40, 513, 7, 100, 2049], 11)
    mask = np.random.default_rng(3).random(s.size) < 0.8
    for gain in ('exp2', 'linear'):
        for m in (None, mask):
            md = None if m is None else _t(m, dev)
            hard, n_hard = in_batch_ndcg(_t(s, dev), _t(y, dev), _t(groups, dev), md, gain)
            loss, n, _ = _run(dev, s, y, groups, m, gain, 1e-4)
            print('tau 1e-4 %s: -loss %.9g, in_batch_ndcg %.9g' % (gain, -float(loss), hard.item()))
            assert n == n_hard.item() and abs(-float(loss) - hard.item()) <= 1e-6


def test_segments_and_repeated_calls_give_the_same_bits(dev):
    name = 'r2048'
    groups, s, y, mask = O.layout(name)
    a = _run(dev, s, y, groups, mask, 'exp2', 0.1)
    b = _run(dev, s, y, groups, mask, 'exp2', 0.1)
    c = _run(dev, s, y, None, mask, 'exp2', 0.1, segments=_segments(_t(groups, dev)))
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes() and a[1] == other[1] and a[2].tobytes() == other[2].tobytes()
    t1, t2 = (_terms(dev, s, y, groups, mask, 0.1) for _ in range(2))
    for x, z in zip(t1, t2):
        assert x.tobytes() == z.tobytes()


def test_the_upstream_gradient_scales(dev):
    groups, s, y, mask = O.layout('r2049')
    _, _, g1 = _run(dev, s, y, groups, mask, 'exp2', 1.0)
    _, _, g2 = _run(dev, s, y, groups, mask, 'exp2', 1.0, upstream=-2.0)
    assert np.abs(g1).max() > 0 and np.array_equal(g2, -2.0 * g1)
    # the loss as a column of a matrix: the gradient has the input's shape
    M = _mod()
    sd = _t(s, dev).reshape(-1, 1).requires_grad_(True)
    M.approx_ndcg_loss(sd, _t(y, dev).reshape(-1, 1), _t(groups, dev), _t(mask, dev), temperature=1.0).backward()
    assert sd.grad.shape == sd.shape and np.array_equal(sd.grad.reshape(-1).cpu().numpy(), g1)


def test_graph_replay_gives_the_eager_bits(dev):
    """Capture and replay of forward and backward.  The eager step runs on a non-default stream and leaves no reference to its autograd graph
    behind, as the capture test of tests/test_listmle_gpu.py does."""
    M = _mod()
    groups, s, y, mask = O.layout('r2048')
    gd, yd, md = _t(groups, dev), _t(y, dev), _t(mask, dev)
    sd = _t(s, dev).requires_grad_(True)

    def step():
        loss, n = M.approx_ndcg_loss(sd, yd, gd, md, return_num_list=True)
        (g,) = torch.autograd.grad(loss, sd)
        return loss.detach(), n, g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [o.clone() for o in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = _ref('r2048', 'one', True, 'exp2', 0.1)
    assert int(eager[1].item()) == ref.n_lists and abs(float(eager[0]) - ref.loss) <= 1e-5
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
    read once).  The grouping then leaves the identity order and n_seg = -1; the kernels stay in bounds on it and the outputs are poisoned."""
    import subprocess
    import sys
    code = r'''
import numpy as np, torch
from rec_now_amd.rec_block import approx_ndcg
dev = torch.device('cuda:0')
rng = np.random.default_rng(0)
B = 20000
y = torch.from_numpy(rng.integers(0, 3, B).astype(np.float32)).to(dev)
s = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev).requires_grad_(True)
g = torch.from_numpy(rng.integers(0, 20, B).astype(np.int64)).to(dev)
loss, n = approx_ndcg.approx_ndcg_loss(s, y, g, return_num_list=True)
loss.backward()
t = approx_ndcg.approx_ndcg_terms(s, y, g)
torch.cuda.synchronize()
assert np.isnan(loss.item()) and n.item() == -1 and bool(torch.isnan(s.grad).all().item()), (loss, n)
assert np.isnan(t.loss_sum.item()) and t.n_lists.item() == -1
print('poisoned ok')
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=root,
                         env=dict(os.environ, RECNOW_DEBUG_GROUP_TIMEOUT='1', PYTHONPATH=root))
    assert out.returncode == 0 and 'poisoned ok' in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]


# ---- containment ------------------------------------------------------------------------------------------------------------------------------
def _all_outputs(dev, s, y, groups, mask, tau=0.1):
    loss, n, grad = _run(dev, s, y, groups, mask, 'exp2', tau)
    return [loss, np.array(n), grad] + _terms(dev, s, y, groups, mask, tau)


@pytest.mark.parametrize('name', ['r2049', 'chain'])
def test_a_nan_score_stays_inside_its_list(dev, name):
    groups, s, y, mask = O.layout(name)
    clean = _ref(name, 'one', True, 'exp2', 0.1)
    l0, n0, g0 = _run(dev, s, y, groups, mask, 'exp2', 0.1)
    sizes = np.array([rows.size for rows in clean.lists])
    for size in (sizes.max(), 600, np.sort(sizes)[2]):                      # the longest list (a wave per row), one of 600 (from LDS), a short one
        g = int(np.flatnonzero(sizes == size)[0])
        rows = clean.lists[g]
        part = rows[np.asarray(mask)[rows]]
        s3 = np.array(s)
        s3[part[part.size // 2]] = NAN
        l3, n3, g3 = _run(dev, s3, y, groups, mask, 'exp2', 0.1)
        in_list = clean.list_id == g
        assert np.isnan(float(l3)) and n3 == n0
        assert np.isnan(g3[part]).all() and (g3[in_list & ~np.asarray(mask)] == 0).all()
        assert g3[~in_list].tobytes() == g0[~in_list].tobytes()
    # a list of one row whose score is NaN: its R is NaN by definition
    s1 = np.array([NAN, 1.0, 2.0], dtype=np.float32)
    loss, n, grad = _run(dev, s1, [1.0, 1.0, 0.0], np.array([0, 1, 1], dtype=np.float32), None, 'exp2', 0.1)
    assert np.isnan(float(loss)) and n == 2 and np.isnan(grad[0]) and np.isfinite(grad[1:]).all()


@pytest.mark.parametrize('name', ['r2048', 'chain'])
def test_rows_that_do_not_take_part_may_hold_anything(dev, name):
    groups, s, y, mask = O.layout(name)
    out = np.flatnonzero(~np.asarray(mask))
    assert out.size > 100
    s0, y0, s2, y2 = (np.array(a) for a in (s, y, s, y))
    s0[out], y0[out] = 0.0, 0.0
    s2[out], y2[out] = NAN, NAN
    s2[out[::3]], y2[out[1::3]] = np.inf, -np.inf
    for tau in (0.1, 1.0):
        zeros = _all_outputs(dev, s0, y0, groups, mask, tau)
        wild = _all_outputs(dev, s2, y2, groups, mask, tau)
        for a, b in zip(zeros, wild):
            assert a.tobytes() == b.tobytes()
    # a NaN label of a taking-part row: its list is invalid, nothing else changes
    ref = _ref(name, 'one', True, 'exp2', 0.1)
    g = int(np.flatnonzero(ref.valid)[1])
    rows = ref.lists[g]
    y3 = np.array(y)
    y3[rows[np.asarray(mask)[rows]][0]] = NAN
    l3, n3, g3 = _run(dev, s, y3, groups, mask, 'exp2', 0.1)
    assert n3 == ref.n_lists - 1 and np.isfinite(float(l3)) and (g3[rows] == 0).all()


def test_c_entry_return_codes(dev):
    from rec_now_amd import _lib
    lib = _lib.load()
    P = _lib.ptr
    groups, s, y, mask = O.layout('r2049')
    seg = _segments(_t(groups, dev))
    sd, yd = _t(s, dev), _t(y, dev)
    B = seg.B
    nbytes = lib.recnow_approx_ndcg_workspace_bytes(B)
    assert nbytes > lib.recnow_pairwise_workspace_bytes(B) and lib.recnow_approx_ndcg_workspace_bytes(-1) == 0
    ws = _lib.workspace(nbytes, dev)
    loss = torch.full((), 7.0, device=dev)
    lsum = torch.full((), 7.0, dtype=torch.float64, device=dev)
    nl = torch.full((), 7, dtype=torch.int64, device=dev)

    def args(n=nbytes, B=B, gain=0, tau=0.1, scores=sd, first=seg.seg_first):
        return (P(scores), P(yd), None, P(seg.order), P(seg.seg_id), P(first), P(seg.n_seg), B, gain, tau, P(loss), P(lsum), P(nl), None, None,
                None, None, P(ws), n, _lib.stream())
    f = lib.recnow_approx_ndcg_fwdbwd
    assert f(*args(n=nbytes - 1)) == EWORKSPACE
    assert f(*args()) == 0                                                          # every per-row and per-list output is optional
    ref = _ref('r2049', 'one', False, 'exp2', 0.1)
    assert nl.item() == ref.n_lists and abs(loss.item() - ref.loss) <= 1e-5 and abs(lsum.item() - ref.loss_sum) <= 1e-6 * abs(ref.loss_sum)
    for bad in (dict(gain=2), dict(gain=-1), dict(tau=0.0), dict(tau=-1.0), dict(tau=NAN), dict(tau=float('inf')), dict(B=-1), dict(scores=None),
                dict(first=None)):
        assert f(*args(**bad)) == EINVAL, bad
    assert f(*args(B=0)) == 0 and loss.item() == 0.0 and lsum.item() == 0.0 and nl.item() == 0

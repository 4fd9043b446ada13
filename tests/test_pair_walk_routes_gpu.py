"""The pair walks of csrc/pairwise_table.hip, csrc/pairwise_kind.hip and csrc/pairwise_lambda.hip (and the base BPR walk beside them) on every
route of csrc/pairwise_walk.hpp, list by list against the per-list fp64 oracle tests/_pair_lists_oracle.py (pinned on the CPU in
tests/test_pair_lists_oracle_cpu.py).

Routes.  Three layouts (O.LAYOUTS) reach, between them, every class of O.CLASSES: a thread per row from the LDS stage and from global memory
(block ranges of exactly 2048 and 2049 members among them), a wave per row from LDS and from global memory, segments of 1 / 2 / 512 / 513 /
2048 / 2049 rows, and every shape of a 64-row block of the wave-per-row kernels that meets two segments.  `test_every_route_class_is_reached`
reads `seg_first` back from `group_rows` and asserts it, so a layout cannot silently stop reaching its route.

Every case goes through `pairwise_loss` as a user calls it, with `pair_indices` (the door to the general route) patched to raise.

Bounds.  Pair count exact; loss within 1e-5 * max(1, |ref|); gradient LIST BY LIST: for every list with a pair, max_i |d_i - ref_i| <=
1e-5 * max_i |ref_i| over the rows of that list -- the project's bound, applied to every list on its own, none left out; rows of lists without
a pair and masked rows exactly 0.  Pre-pass: positions exact, discount / gain / inv_idcg within 1e-6 relative (exactly 0 where the reference
is), per-list DCG and IDCG of the C entry within 1e-12 relative, the mean within 1e-6, the list count exact.  `cnt_row` of both count entries
exact.  Each case prints its worst per-list ratio err / (1e-5 * scale); DESIGN.md 8o holds the worst per family as measured.

Hinge cases run with margin = m + 2**-10 and power-of-two factors, and each asserts from the fp64 values that no candidate of a list lies
within 2**-10 of the kink."""
import functools

import numpy as np
import pytest
import torch

import _pair_lists_oracle as O
from _pair_lists_oracle import no_general_route as _no_general_route

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FAR = 10000                                      # a topn beyond every list
FLAG_LABEL_GT, FLAG_WRONG_ORDER = 1, 2           # RECNOW_PAIR_LABEL_GT, RECNOW_PAIR_WRONG_ORDER of include/recnow.h
NAMES = tuple(O.LAYOUTS)


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _ndcg():
    from rec_now_amd.rec_block import ndcg
    return ndcg


def _t(a):
    return torch.from_numpy(np.array(a))         # a copy: the shared layouts and references stay as they are


def _groups(name, variant):
    g = O.layout(name)[0]
    return [g, O.second_groups(g.size)] if variant == 'two' else g


def _dev_groups(g, dev):
    return [_t(t).to(dev) for t in g] if isinstance(g, list) else _t(g).to(dev)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
# margin and factor of each pair loss: the hinge kind sits half a grid step off every kink and takes power-of-two factors only
OPTIONS = {'bpr': (0.0, 1.0), 'hinge': (1.0 + O.KINK, 0.5), 'squared_hinge': (0.5, 0.7), 'margin_bpr': (0.3, 2.0)}
WALK_KINDS = ('hinge', 'squared_hinge', 'margin_bpr')          # the KIND parameter of the kind and the NDCG walks


def _case(family, kind, rule, wrong, lam=None, power=0.0, reduce_mean=True, variant='one', use_mask=True):
    return (family, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask)


# rule: 'default' -- no table, label_i > label_j; 'table' -- the same rule as a LabelPairWeightTable; 'sym' -- the table of w_sym
EVERY_LAYOUT = (
    [_case('base', 'bpr', 'default', False)]
    + [_case('table', 'bpr', r, w) for r in ('table', 'sym') for w in (False, True)]
    + [_case('kind', k, r, w) for k in WALK_KINDS for r in ('default', 'sym') for w in (False, True)]                       # <KIND, TABLE, WRONG>
    + [_case('lambda', k, r, w, ('exp2', None)) for k in WALK_KINDS for r in ('default', 'sym') for w in (False, True)]     # <KIND, TABLE, WRONG>
    + [_case('lambda', 'bpr', 'default', False, ('linear', None)), _case('lambda', 'bpr', 'sym', False, ('exp2', 5)),
       _case('lambda', 'bpr', 'default', True, ('exp2', FAR))])
ONE_LAYOUT = {
    'r2049': [_case('base', 'bpr', 'default', False, power=-0.5), _case('table', 'bpr', 'sym', False, power=-0.5),
              _case('kind', 'hinge', 'default', False, power=-0.5), _case('lambda', 'margin_bpr', 'sym', False, ('exp2', None), power=-0.5),
              _case('base', 'bpr', 'default', False, use_mask=False), _case('table', 'bpr', 'sym', False, use_mask=False),
              _case('kind', 'squared_hinge', 'default', False, use_mask=False),
              _case('lambda', 'hinge', 'sym', True, ('exp2', None), use_mask=False)],
    'r2048': [_case('base', 'bpr', 'default', True, power=1.0), _case('table', 'bpr', 'table', True, power=1.0),
              _case('kind', 'squared_hinge', 'sym', False, power=1.0), _case('lambda', 'hinge', 'default', False, ('exp2', None), power=1.0)],
    'chain': [_case('base', 'bpr', 'default', False, reduce_mean=False), _case('table', 'bpr', 'sym', False, reduce_mean=False),
              _case('kind', 'margin_bpr', 'default', False, reduce_mean=False),
              _case('lambda', 'squared_hinge', 'sym', False, ('exp2', None), reduce_mean=False),
              # a second group tensor: three times as many lists, and the occurrence count of a main group now spans several of them
              _case('base', 'bpr', 'default', False, power=-0.5, variant='two'), _case('table', 'bpr', 'sym', False, power=-0.5, variant='two'),
              _case('kind', 'hinge', 'sym', True, power=-0.5, variant='two'),
              _case('lambda', 'bpr', 'default', False, ('exp2', None), power=-0.5, variant='two')],
}
CASES = [(n,) + c for n in NAMES for c in EVERY_LAYOUT + ONE_LAYOUT[n]]


def _case_id(c):
    name, family, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask = c
    bits = [name, family, kind, rule, 'wrong' if wrong else 'all']
    if lam is not None:
        bits.append('%s-%s' % lam)
    if power:
        bits.append('pow%g' % power)
    bits += [w for w, on in (('sum', not reduce_mean), ('two', variant == 'two'), ('nomask', not use_mask)) if on]
    return '-'.join(bits)


# ---- references (computed once, shared, read-only) ---------------------------------------------------------------------------------------
_STRUCT, _ORACLE, _OFF_KINK = {}, {}, set()


def _rule_fn(rule):
    return O.w_sym if rule == 'sym' else None                # 'table' is the default rule written as a table


def _structure(name, variant, rule, wrong, use_mask):
    key = (name, variant, _rule_fn(rule) is not None, wrong, use_mask)
    if key not in _STRUCT:
        _, s, y, mask = O.layout(name)
        _STRUCT[key] = O.structure(s, y, _groups(name, variant), _rule_fn(rule), wrong, mask if use_mask else None)
    return _STRUCT[key]


def _oracle(name, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask):
    margin, factor = OPTIONS[kind]
    key = (name, variant, _rule_fn(rule) is not None, wrong, use_mask, power, kind, margin, factor, lam, reduce_mean)
    if key not in _ORACLE:
        _, s, y, mask = O.layout(name)
        _ORACLE[key] = O.pairwise_loss(s, y, _groups(name, variant), kind, margin, factor, reduce_mean, _rule_fn(rule), wrong, power,
                                       mask if use_mask else None, lam, pairs=_structure(name, variant, rule, wrong, use_mask))
    return _ORACLE[key]


def _assert_off_the_kink(name, variant, margin, factor):
    if (name, variant, margin, factor) not in _OFF_KINK:
        O.assert_off_the_kink(_groups(name, variant), O.layout(name)[1], margin, factor)
        _OFF_KINK.add((name, variant, margin, factor))


# ---- running a case ------------------------------------------------------------------------------------------------------------------------
def _pairloss(M, kind, reduce_mean):
    margin, factor = OPTIONS[kind]
    if kind == 'bpr':
        return functools.partial(M.bpr_loss_func, factor=factor, reduce_mean=reduce_mean)
    f = {'hinge': M.hinge_loss_func, 'squared_hinge': M.squared_hinge_loss_func, 'margin_bpr': M.margin_bpr_loss_func}[kind]
    return functools.partial(f, margin=margin, factor=factor, reduce_mean=reduce_mean)


def _run(M, dev, name, family, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask):
    _, s, y, mask = O.layout(name)
    kw = {}
    if family != 'base':
        kw['pairloss_func'] = _pairloss(M, kind, reduce_mean)
    elif not reduce_mean:
        kw['pairloss_func'] = functools.partial(M.bpr_loss_func, reduce_mean=False)
    if rule != 'default':
        kw['label_pair_to_weight_func'] = M.LabelPairWeightTable(O.LEVELS, O.w_sym) if rule == 'sym' else M.LabelPairWeightTable(O.LEVELS)
    if lam is not None:
        kw['lambda_weight'] = _ndcg().NDCGLambdaWeight(gain=lam[0], topn=lam[1])
    sd = _t(s).to(dev).requires_grad_(True)
    loss, n_pair = M.pairwise_loss(sd, _t(y).to(dev), _dev_groups(_groups(name, variant), dev), only_use_wrong_order_pair=wrong,
                                   return_num_pair=True, click_occurance_power=power, mask=_t(mask).to(dev) if use_mask else None, **kw)
    loss.backward()
    return loss.item(), n_pair.item(), sd.grad.cpu().numpy()


def _check(got, ref, mask, what):
    """pair count, loss, and the gradient inside every list; returns the worst err / (RTOL * scale) over the lists"""
    loss, n_pair, grad = got
    assert n_pair == ref.n_pair                                        # integer path: exact
    assert ref.n_pair > 0
    worst, worst_n = 0.0, 0
    bad = []
    silent = np.zeros(grad.size, dtype=bool) if mask is None else ~mask
    for l in ref.lists:
        if l.n_pair == 0:
            silent[l.rows] = True
            continue
        err = float(np.abs(grad[l.rows] - ref.grad[l.rows]).max())
        scale = float(np.abs(ref.grad[l.rows]).max())
        ratio = err / (RTOL * scale) if scale > 0 else (0.0 if err == 0 else float('inf'))
        if ratio > worst:
            worst, worst_n = ratio, l.rows.size
        if not err <= RTOL * scale:
            bad.append((l.rows.size, err, scale))
    print('ROUTES %s: n_pair %d  loss %.9g (ref %.9g, err %.3g)  worst list ratio %.4f of the bound (a list of %d rows)'
          % (what, n_pair, loss, ref.loss, abs(loss - ref.loss), worst, worst_n))
    assert abs(loss - ref.loss) <= RTOL * max(1.0, abs(ref.loss))
    assert not bad, 'lists (rows, err, scale) beyond 1e-5 of themselves: %s' % bad[:8]
    assert not grad[silent].any()                                      # lists without a pair and masked rows: exactly 0
    return worst


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_route_case_list_by_list(dev, monkeypatch, case):
    M = _mod()
    _no_general_route(monkeypatch, M)
    name, family, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask = case
    if kind == 'hinge':
        margin, factor = OPTIONS[kind]
        assert factor in (0.5, 1.0, 2.0)
        _assert_off_the_kink(name, variant, margin, factor)
    got = _run(M, dev, *case)
    ref = _oracle(name, kind, rule, wrong, lam, power, reduce_mean, variant, use_mask)
    _check(got, ref, O.layout(name)[3] if use_mask else None, _case_id(case))


# ---- census --------------------------------------------------------------------------------------------------------------------------------
def test_every_route_class_is_reached(dev):
    """From the segments the library itself builds: the sizes in sorted order are the layout's, and every class of routes is non-empty in at
    least one layout."""
    M = _mod()
    got = {}
    for name in NAMES:
        g = O.layout(name)[0]
        seg = M.group_rows(_t(g).to(dev))
        assert seg.B == g.size
        sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), seg.B)
        assert np.diff(sf).tolist() == O.LAYOUTS[name] and sf.size - 1 == seg.num_segments()
        got[name] = O.census(seg.seg_first.cpu().numpy(), seg.B)
        print('ROUTES census %s: %s' % (name, got[name]))
    for cls in O.CLASSES:
        assert any(c[cls] > 0 for c in got.values()), 'no layout reaches %s' % cls
    assert got['r2049']['t_range_2049'] and got['r2049']['t_global'] and got['r2048']['t_range_2048'] and got['r2048']['t_global']


# ---- NDCG pre-pass -------------------------------------------------------------------------------------------------------------------------
def _rel_ok(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref)
    nz = ref != 0
    worst = float((err[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0
    print('ROUTES %s: worst relative error %.3g' % (what, worst))
    assert (err <= tol * np.abs(ref)).all(), what                    # a reference of exactly 0 (no position, cut off, IDCG = 0) must be exactly 0


@pytest.mark.parametrize('name,use_mask', [(n, True) for n in NAMES] + [('r2049', False)])
def test_ndcg_prepass_row_by_row_and_list_by_list(dev, name, use_mask):
    from rec_now_amd import _lib
    M, N = _mod(), _ndcg()
    g, s, y, mask = O.layout(name)
    m = mask if use_mask else None
    gd, sd, yd = _t(g).to(dev), _t(s).to(dev), _t(y).to(dev)
    md = _t(mask).to(dev) if use_mask else None
    m8 = None if md is None else md.to(torch.uint8).contiguous()
    seg = M.group_rows(gd)
    B = seg.B
    order = seg.order.cpu().numpy()
    sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), B)
    lib = _lib.load()
    for gain, topn in (('exp2', None), ('linear', 5), ('exp2', FAR)):
        ref = O.rank_terms(s, y, g, m, gain, topn)
        what = '%s %s %s-%s' % (name, 'mask' if use_mask else 'nomask', gain, topn)
        got = N.ndcg_rank_terms(sd, yd, gd, mask=md, gain=gain, topn=topn)
        assert np.array_equal(got.rank.cpu().numpy().astype(np.int64), ref.rank)
        _rel_ok(got.discount.cpu().numpy(), ref.discount, 1e-6, what + ' discount')
        _rel_ok(got.gain.cpu().numpy(), ref.gain, 1e-6, what + ' gain')
        _rel_ok(got.inv_idcg.cpu().numpy(), ref.inv_idcg, 1e-6, what + ' inv_idcg')
        mean, n_lists = N.in_batch_ndcg(sd, yd, None, mask=md, gain=gain, topn=topn, segments=seg)
        print('ROUTES %s: NDCG %.9g (ref %.9g) over %d lists (ref %d)' % (what, mean.item(), ref.ndcg_mean, n_lists.item(), ref.n_lists))
        assert n_lists.item() == ref.n_lists
        assert abs(mean.item() - ref.ndcg_mean) <= 1e-6
        # the C entry hands out every list's DCG and IDCG in fp64, by segment
        dcg = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
        idcg = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
        ws = N.lambda_workspace(B, dev)
        rc = lib.recnow_pair_lambda_terms(_lib.ptr(sd), _lib.ptr(yd), _lib.ptr(m8), _lib.ptr(seg.order), _lib.ptr(seg.seg_id),
                                          _lib.ptr(seg.seg_first), B, 0, {'exp2': 0, 'linear': 1}[gain], int(topn or 0), None, None, None, None,
                                          _lib.ptr(dcg), _lib.ptr(idcg), None, None, _lib.ptr(ws), ws.numel(), _lib.stream())
        assert rc == 0
        dcg, idcg = dcg.cpu().numpy(), idcg.cpu().numpy()
        lists = O.rows_of_lists(ref.list_id)
        want_d, want_i = np.zeros(sf.size - 1), np.zeros(sf.size - 1)
        for k in range(sf.size - 1):
            rows = np.sort(order[sf[k]:sf[k + 1]])
            lid = int(ref.list_id[rows[0]])
            assert np.array_equal(rows, lists[lid])                    # a segment is a list
            want_d[k], want_i[k] = ref.dcg[lid], ref.idcg[lid]
        _rel_ok(dcg[:sf.size - 1], want_d, 1e-12, what + ' list DCG')
        _rel_ok(idcg[:sf.size - 1], want_i, 1e-12, what + ' list IDCG')


# ---- the count entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrong', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_cnt_row_of_both_count_entries(dev, name, wrong):
    """cnt_row by ORIGINAL row index (include/recnow.h): the number of pairs the row is the positive of."""
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, mask = O.layout(name)
    seg = M.group_rows(_t(g).to(dev))
    B = seg.B
    sd, yd, m8 = _t(s).to(dev), _t(y).to(dev), _t(mask).to(dev).to(torch.uint8).contiguous()
    P, st = _lib.ptr, _lib.stream()
    ws = _lib.workspace(_lib.load().recnow_pairwise_workspace_bytes(B), dev)
    vals, w = M.LabelPairWeightTable(O.LEVELS, O.w_sym).on_device(dev)
    for rule in ('default', 'sym'):
        cnt_row = torch.full((B,), -1, dtype=torch.int32, device=dev)
        cnt_super = torch.empty(B, dtype=torch.int64, device=dev)
        n_pair = torch.full((1,), -1, dtype=torch.int64, device=dev)
        if rule == 'sym':
            _lib.call('recnow_pair_table_count', P(sd), P(yd), P(m8), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), B,
                      FLAG_WRONG_ORDER if wrong else 0, P(vals), 4, P(w), P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
        else:
            _lib.call('recnow_pair_count', P(sd), P(yd), P(m8), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), B,
                      FLAG_LABEL_GT | (FLAG_WRONG_ORDER if wrong else 0), P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
        ref = _structure(name, 'one', rule, wrong, True)
        got = cnt_row.cpu().numpy().astype(np.int64)
        assert n_pair.item() == ref.n_pair > 0
        diff = np.flatnonzero(got != ref.cnt_row)
        assert diff.size == 0, '%s: %d rows differ, first %s' % (rule, diff.size, diff[:8])
        # per main group: one list is one main group here
        cs = cnt_super.cpu().numpy()[:len(ref.lists)]
        assert sorted(cs.tolist()) == sorted(ref.cnt_list.tolist())


# ---- repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c[0] == 'chain' and c[1:] in (
    _case('base', 'bpr', 'default', False), _case('table', 'bpr', 'sym', True), _case('kind', 'margin_bpr', 'sym', False),
    _case('lambda', 'hinge', 'default', True, ('exp2', None)))], ids=_case_id)
def test_run_to_run_bit_identical(dev, monkeypatch, case):
    M = _mod()
    _no_general_route(monkeypatch, M)
    a, b = _run(M, dev, *case), _run(M, dev, *case)
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1] == b[1] > 0
    assert a[2].tobytes() == b[2].tobytes() and np.abs(a[2]).max() > 0

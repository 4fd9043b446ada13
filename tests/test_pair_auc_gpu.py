"""In-batch GAUC (rec_block/auc.py, csrc/pairwise_auc.hip) on every route of csrc/pairwise_walk.hpp against the list-by-list integer oracle
tests/_auc_oracle.py (pinned on the CPU in tests/test_auc_oracle_cpu.py).

Routes.  The three layouts of tests/_pair_lists_oracle.py (r2049, r2048, chain: 3513 to 6425 rows) reach, between them, every class of
O.CLASSES; `test_every_route_class_is_reached` reads `seg_first` back from `group_rows` and asserts it.

Bounds.  Per-row counts n_i, c_i, t_i exact for every row; per-list N, C, T, R exact for every segment, no list left out; the metric within
1e-6 relative for each weight (one float32 rounding of an fp64 ratio: the bound in_batch_ndcg is held to); its fp64 numerator and denominator
within 1e-12 relative (at most a few dozen fp64 terms); the number of lists exact.  Every case asserts from the oracle alone that its batch
holds a list without a pair, a list with tied pairs and, under the graded rule, a list with concordant and discordant pairs."""
import numpy as np
import pytest
import torch

import _auc_oracle as A
import _pair_lists_oracle as O

pytestmark = pytest.mark.gpu

NAMES = tuple(O.LAYOUTS)
FLAG_LABEL_GT, FLAG_MEMBERS_PACKED = 1, 256      # RECNOW_PAIR_LABEL_GT, RECNOW_PAIR_MEMBERS_PACKED of include/recnow.h
EINVAL, EWORKSPACE = -1, -2                      # RECNOW_EINVAL, RECNOW_EWORKSPACE
WEIGHT_CODE = {'rows': 0, 'pairs': 1, 'uniform': 2}
NAN = float('nan')
ROW_FIELDS = (('row_pairs', 'row_n'), ('row_concordant', 'row_c'), ('row_tied', 'row_t'))
LIST_FIELDS = (('list_pairs', 'N'), ('list_concordant', 'C'), ('list_tied', 'T'), ('list_rows', 'R'))


def _mod():
    from rec_now_amd.rec_block import pairwise_loss_from_batch as M
    return M


def _auc():
    from rec_now_amd.rec_block import auc
    return auc


def _t(a):
    return torch.from_numpy(np.array(a))         # a copy: the shared layouts and references stay as they are


def _groups(name, variant):
    g = O.layout(name)[0]
    return [g, O.second_groups(g.size)] if variant == 'two' else g


def _dev_groups(g, dev):
    return [_t(t).to(dev) for t in g] if isinstance(g, list) else _t(g).to(dev)


# ---- references (computed once, shared, read-only) ---------------------------------------------------------------------------------------
_REF = {}


def _ref(name, variant, use_mask, th):
    key = (name, variant, use_mask, th)
    if key not in _REF:
        _, s, y, mask = O.layout(name)
        _REF[key] = A.counts(s, y, _groups(name, variant), mask if use_mask else None, th)
    return _REF[key]


def _lists_of_segments(seg, cnt):
    """for every segment of the library the oracle's list it is (a segment IS a list: the same rows); every list appears once"""
    B = seg.B
    order = seg.order.cpu().numpy()
    sf = O.trim_seg_first(seg.seg_first.cpu().numpy(), B)
    n_seg = sf.size - 1
    assert n_seg == len(cnt.lists) == seg.num_segments()
    lid = np.empty(n_seg, dtype=np.int64)
    for k in range(n_seg):
        rows = np.sort(order[sf[k]:sf[k + 1]])
        lid[k] = cnt.list_id[rows[0]]
        assert np.array_equal(rows, cnt.lists[lid[k]])
    assert np.unique(lid).size == n_seg
    return lid


def _check_terms(got, ref, lid, what):
    for field, name in ROW_FIELDS:
        have = getattr(got, field)
        assert have.dtype == torch.int32 and have.shape == (ref.row_n.size,)
        diff = np.flatnonzero(have.cpu().numpy().astype(np.int64) != getattr(ref, name))
        assert diff.size == 0, '%s %s: %d rows differ, first %s' % (what, field, diff.size, diff[:8])
    for field, name in LIST_FIELDS:
        have = getattr(got, field)
        assert have.dtype == torch.int64 and have.shape == (ref.row_n.size,)
        want = getattr(ref, name)[lid]
        diff = np.flatnonzero(have.cpu().numpy()[:lid.size] != want)
        assert diff.size == 0, '%s %s: %d segments differ, first %s' % (what, field, diff.size, diff[:8])


def _check_metric(got, want, what):
    assert (got.auc.dtype, got.n_lists.dtype, got.weighted_sum.dtype, got.weight_sum.dtype) == (torch.float32, torch.int64, torch.float64,
                                                                                                torch.float64)
    assert got.auc.shape == got.n_lists.shape == got.weighted_sum.shape == got.weight_sum.shape == ()
    auc, n, num, den = got.auc.item(), got.n_lists.item(), got.weighted_sum.item(), got.weight_sum.item()
    print('AUC %s: %.9g (ref %.9g, rel err %.3g) over %d lists (ref %d); sums rel err %.3g, %.3g'
          % (what, auc, want.auc, abs(auc - want.auc) / max(abs(want.auc), 1e-300), n, want.n_lists,
             abs(num - want.weighted_sum) / max(abs(want.weighted_sum), 1e-300), abs(den - want.weight_sum) / max(abs(want.weight_sum), 1e-300)))
    assert n == want.n_lists
    assert abs(auc - want.auc) <= 1e-6 * abs(want.auc)
    assert abs(num - want.weighted_sum) <= 1e-12 * abs(want.weighted_sum)
    assert abs(den - want.weight_sum) <= 1e-12 * abs(want.weight_sum)


def _assert_batch_is_telling(ref, graded):
    """from the oracle alone"""
    assert (ref.N == 0).any()                                          # a list without a pair: left out of the mean
    assert (ref.T > 0).any()                                           # tied pairs
    if graded:
        assert ((ref.C > 0) & (ref.N - ref.C - ref.T > 0)).any()       # concordant and discordant pairs in one list


# ---- every route, every rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['one', 'two'])
@pytest.mark.parametrize('th', [None, 0.5, 1.5], ids=['graded', 'th0.5', 'th1.5'])
@pytest.mark.parametrize('use_mask', [True, False], ids=['mask', 'nomask'])
@pytest.mark.parametrize('name', NAMES)
def test_counts_and_metric_list_by_list(dev, name, use_mask, th, variant):
    M, AUC = _mod(), _auc()
    ref = _ref(name, variant, use_mask, th)
    _assert_batch_is_telling(ref, th is None)
    _, s, y, mask = O.layout(name)
    sd, yd = _t(s).to(dev), _t(y).to(dev)
    md = _t(mask).to(dev) if use_mask else None
    gd = _dev_groups(_groups(name, variant), dev)
    seg = M.group_rows(gd)
    what = '%s %s %s %s' % (name, 'mask' if use_mask else 'nomask', th, variant)
    got = AUC.auc_terms(sd, yd, None, mask=md, pos_neg_th=th, segments=seg)
    _check_terms(got, ref, _lists_of_segments(seg, ref), what)
    for w in A.WEIGHTS:
        res = AUC.in_batch_gauc(sd, yd, gd, mask=md, pos_neg_th=th, weight=w, segments=None if w == 'rows' else seg)
        _check_metric(res, A.metric(ref, w), what + ' ' + w)


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
    for cls in O.CLASSES:
        assert any(c[cls] > 0 for c in got.values()), 'no layout reaches %s' % cls
    assert got['r2049']['t_range_2049'] and got['r2049']['t_global'] and got['r2048']['t_range_2048'] and got['r2048']['t_global']


# ---- consistency with the shipped pair counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_totals_equal_the_pair_counts_of_the_loss(dev, name):
    """sum N = the pair count of the default rule; sum (N - C - T) = the pair count under only_use_wrong_order_pair (s_i < s_j: the layouts
    have no NaN score).  The loss reports its count as float32: exact below 2**24."""
    M, AUC = _mod(), _auc()
    g, s, y, mask = O.layout(name)
    gd, sd, yd, md = _t(g).to(dev), _t(s).to(dev), _t(y).to(dev), _t(mask).to(dev)
    ref = _ref(name, 'one', True, None)
    got = AUC.auc_terms(sd, yd, gd, mask=md)
    n_seg = len(ref.lists)
    total = int(got.list_pairs[:n_seg].sum().item())
    wrong = int((got.list_pairs - got.list_concordant - got.list_tied)[:n_seg].sum().item())
    assert total == int(ref.N.sum()) and wrong == int((ref.N - ref.C - ref.T).sum()) and 0 < wrong < total < 2 ** 24
    _, n_all = M.pairwise_loss_fused(sd, yd, gd, mask=md)
    _, n_wrong = M.pairwise_loss_fused(sd, yd, gd, mask=md, only_use_wrong_order_pair=True)
    assert n_all.item() == float(total) and n_wrong.item() == float(wrong)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------------
def _c_call(dev, seg, sd, yd, m8, flags, binary, th, weight, ws, nbytes=None):
    """every output of recnow_pair_auc_terms, as host arrays, from buffers filled with -1 / NaN beforehand; the return code first"""
    from rec_now_amd import _lib
    B, P = seg.B, _lib.ptr
    rows = [torch.full((max(B, 1),), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    lists = [torch.full((max(B, 1),), -1, dtype=torch.int64, device=dev) for _ in range(4)]
    auc = torch.full((1,), NAN, dtype=torch.float32, device=dev)
    num, den = (torch.full((1,), NAN, dtype=torch.float64, device=dev) for _ in range(2))
    n_lists = torch.full((1,), -1, dtype=torch.int64, device=dev)
    outs = rows + lists + [auc, num, den, n_lists]
    rc = _lib.load().recnow_pair_auc_terms(P(sd), P(yd), P(m8), P(seg.order), P(seg.seg_id), P(seg.seg_first), B, flags, binary, th, weight,
                                            *[P(t) for t in outs], P(ws), ws.numel() if nbytes is None else nbytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize('binary,th', [(0, 0.0), (1, 0.5)], ids=['graded', 'th0.5'])
@pytest.mark.parametrize('name', NAMES)
def test_members_packed_by_the_count_call_are_reused(dev, name, binary, th):
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, mask = O.layout(name)
    seg = M.group_rows(_t(g).to(dev))
    B = seg.B
    sd, yd, m8 = _t(s).to(dev), _t(y).to(dev), _t(mask).to(dev).to(torch.uint8).contiguous()
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream()
    nbytes = lib.recnow_pair_auc_workspace_bytes(B)
    assert nbytes > lib.recnow_pairwise_workspace_bytes(B)
    rc, plain = _c_call(dev, seg, sd, yd, m8, 0, binary, th, 0, _lib.workspace(nbytes, dev))
    assert rc == 0
    ws = _lib.workspace(nbytes, dev)
    cnt_row = torch.empty(B, dtype=torch.int32, device=dev)
    cnt_super = torch.empty(B, dtype=torch.int64, device=dev)
    n_pair = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call('recnow_pair_count', P(sd), P(yd), P(m8), P(seg.order), P(seg.seg_id), P(seg.seg_first), P(seg.super_id), B, FLAG_LABEL_GT,
              P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
    rc, packed = _c_call(dev, seg, None, None, None, FLAG_MEMBERS_PACKED, binary, th, 0, ws)
    assert rc == 0
    for a, b in zip(plain, packed):
        assert a.tobytes() == b.tobytes()
    ref = _ref(name, 'one', True, 0.5 if binary else None)
    assert np.array_equal(plain[0].astype(np.int64), ref.row_n) and plain[10][0] == A.metric(ref, 'rows').n_lists > 0
    if not binary:
        assert n_pair.item() == int(ref.N.sum())


def test_c_entry_refuses_bad_arguments(dev):
    """return codes only: every refusal comes before the first launch"""
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, _ = O.layout('r2049')
    seg = M.group_rows(_t(g).to(dev))
    sd, yd = _t(s).to(dev), _t(y).to(dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.recnow_pair_auc_workspace_bytes(seg.B), dev)

    def rc(flags=0, binary=0, th=0.0, weight=0, nbytes=None):
        return _c_call(dev, seg, sd, yd, None, flags, binary, th, weight, ws, nbytes)[0]
    assert rc(weight=3) == EINVAL and rc(weight=-1) == EINVAL
    assert rc(flags=1) == EINVAL and rc(flags=256 | 2) == EINVAL
    assert rc(binary=1, th=NAN) == EINVAL and rc(binary=1, th=float('inf')) == EINVAL
    assert rc(nbytes=lib.recnow_pairwise_workspace_bytes(seg.B)) == EWORKSPACE
    assert lib.recnow_pair_auc_terms(None, None, None, None, None, None, seg.B, 0, 0, 0.0, 0, *([None] * 11), _lib.ptr(ws), ws.numel(),
                                     _lib.stream()) == EINVAL               # NULL segment arrays with B > 0
    assert lib.recnow_pair_auc_workspace_bytes(-1) == 0


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------------
def _one(dev, s, y, g, mask=None, th=None, weight='rows'):
    AUC = _auc()
    dv = lambda a: None if a is None else (a.to(dev) if isinstance(a, torch.Tensor) else _t(a).to(dev))      # noqa: E731
    return (AUC.in_batch_gauc(dv(s), dv(y), dv(g), mask=dv(mask), pos_neg_th=th, weight=weight),
            AUC.auc_terms(dv(s), dv(y), dv(g), mask=dv(mask), pos_neg_th=th))


def _zero_metric(res):
    return (res.auc.item(), res.n_lists.item(), res.weighted_sum.item(), res.weight_sum.item()) == (0.0, 0, 0.0, 0.0)


def test_empty_batch_and_single_row(dev):
    z = np.zeros(0, dtype=np.float32)
    res, terms = _one(dev, z, z, z)
    assert _zero_metric(res) and all(t.shape == (0,) for t in terms)
    from rec_now_amd import _lib
    zd = _t(z).to(dev)
    rc, outs = _c_call(dev, _mod().group_rows(zd), zd, zd, None, 0, 0, 0.0, 0, _lib.workspace(16, dev))      # over buffers of NaN and -1
    assert rc == 0 and [float(o[0]) for o in outs[7:]] == [0.0, 0.0, 0.0, 0.0]
    one = np.ones(1, dtype=np.float32)
    res, terms = _one(dev, one, one, one)
    assert _zero_metric(res)
    assert [t.item() for t in terms] == [0, 0, 0, 0, 0, 0, 1]                      # one list of one row, no pair


def test_every_row_masked_out(dev):
    g, s, y, _ = O.layout('r2049')
    res, terms = _one(dev, s, y, g, mask=np.zeros(g.size, dtype=bool))
    assert _zero_metric(res)
    n_seg = len(O.LAYOUTS['r2049'])                                                # the entries behind the segments are not written
    assert not any(t.any().item() for t in terms[:3]) and not any(t[:n_seg].any().item() for t in terms[3:])      # every count, every list's rows: 0


@pytest.mark.parametrize('weight', A.WEIGHTS)
def test_all_scores_equal_is_exactly_half(dev, weight):
    rng = np.random.default_rng(3)
    y = rng.integers(0, 4, 700).astype(np.float32)
    res, terms = _one(dev, np.full(700, 0.25, dtype=np.float32), y, np.zeros(700, dtype=np.float32), weight=weight)
    assert res.auc.item() == 0.5 and res.n_lists.item() == 1
    N = int(terms.list_pairs[0].item())
    assert N == int((y[:, None] > y[None, :]).sum()) and terms.list_tied[0].item() == N and terms.list_concordant[0].item() == 0


@pytest.mark.parametrize('th', [None, 1.5], ids=['graded', 'th1.5'])
@pytest.mark.parametrize('sign,want', [(1.0, 1.0), (-1.0, 0.0)], ids=['ordered', 'reversed'])
def test_perfect_orders_are_exactly_one_and_zero(dev, sign, want, th):
    """lists of 5, 600 (a wave per row) and 64 rows whose scores follow (or oppose) the labels strictly"""
    rng = np.random.default_rng(4)
    g = np.repeat(np.arange(3), [5, 600, 64]).astype(np.float32)
    rng.shuffle(g)
    y = rng.integers(0, 4, g.size).astype(np.float32)
    s = (sign * (y + 0.125)).astype(np.float32)
    ref = A.counts(s, y, g, None, th)
    assert (ref.N > 0).all() and ref.T.sum() == 0
    for weight in A.WEIGHTS:
        res, terms = _one(dev, s, y, g, th=th, weight=weight)
        assert res.auc.item() == want and res.n_lists.item() == 3
    assert np.array_equal(terms.row_pairs.cpu().numpy(), ref.row_n)
    assert np.array_equal(terms.row_concordant.cpu().numpy(), ref.row_n if want else 0 * ref.row_n)
    assert not terms.row_tied.any().item()


def test_nan_score_and_nan_label(dev):
    """a NaN score in a taking-part row: its pairs are discordant from either side; a NaN label: no pair under the graded rule, a negative
    under the binary rule.  One short list and one list of 600 rows."""
    rng = np.random.default_rng(6)
    g = np.repeat(np.arange(2), [9, 600]).astype(np.float32)
    rng.shuffle(g)
    y = rng.integers(0, 3, g.size).astype(np.float32)
    s = (np.round(rng.normal(size=g.size) * 16) / 16).astype(np.float32)
    for grp in (0, 1):
        rows = np.flatnonzero(g == grp)
        s[rows[np.flatnonzero(y[rows] == 1)[:2]]] = np.nan                    # NaN scores on the higher and on the lower side of pairs
        y[rows[np.flatnonzero(y[rows] == 2)[0]]] = np.nan
    for th in (None, 0.5):
        ref = A.counts(s, y, g, None, th)
        nan_rows = np.flatnonzero(np.isnan(s))
        assert ref.row_n[nan_rows].sum() > 0 and ref.row_c[nan_rows].sum() == 0 and ref.row_t[nan_rows].sum() == 0
        res, terms = _one(dev, s, y, g, th=th)
        seg = _mod().group_rows(_t(g).to(dev))
        _check_terms(terms, ref, _lists_of_segments(seg, ref), 'nan %s' % th)
        _check_metric(res, A.metric(ref, 'rows'), 'nan %s' % th)


@pytest.mark.parametrize('dtype', [torch.int64, torch.float64], ids=['int64', 'float64'])
def test_id_dtypes_and_column_outputs(dev, dtype):
    """an int64 / float64 id tensor whose values a float32 would merge, and outputs, labels and mask of shape (B, 1)"""
    rng = np.random.default_rng(8)
    B = 300
    small = rng.integers(0, 5, B)
    ids = (2 ** 40 + small) if dtype == torch.int64 else (1.0 + small * 2.0 ** -40)
    s = (np.round(rng.normal(size=B) * 4) / 4).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.float32)
    mask = rng.random(B) < 0.9
    ref = A.counts(s, y, small, mask)
    assert len(ref.lists) == 5 and (ref.N > 0).all() and ref.T.sum() > 0
    AUC = _auc()
    gd = torch.from_numpy(np.asarray(ids)).to(dtype).to(dev)
    sd, yd, md = (_t(a).to(dev).reshape(B, 1) for a in (s, y, mask))
    terms = AUC.auc_terms(sd, yd, gd, mask=md)
    seg = _mod().group_rows(gd)
    _check_terms(terms, ref, _lists_of_segments(seg, ref), str(dtype))
    _check_metric(AUC.in_batch_gauc(sd, yd, gd.reshape(B, 1), mask=md, weight='uniform'), A.metric(ref, 'uniform'), str(dtype))


# ---- repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('th', [None, 0.5], ids=['graded', 'th0.5'])
def test_run_to_run_bit_identical(dev, th):
    from rec_now_amd import _lib
    M = _mod()
    g, s, y, mask = O.layout('chain')
    seg = M.group_rows(_t(g).to(dev))
    sd, yd, m8 = _t(s).to(dev), _t(y).to(dev), _t(mask).to(dev).to(torch.uint8).contiguous()
    nbytes = _lib.load().recnow_pair_auc_workspace_bytes(seg.B)
    runs = [_c_call(dev, seg, sd, yd, m8, 0, 0 if th is None else 1, th or 0.0, 0, _lib.workspace(nbytes, dev)) for _ in range(2)]
    assert runs[0][0] == runs[1][0] == 0
    for a, b in zip(runs[0][1], runs[1][1]):
        assert a.tobytes() == b.tobytes()
    assert runs[0][1][0].max() > 0 and runs[0][1][10][0] > 0 and 0.0 < runs[0][1][7][0] < 1.0

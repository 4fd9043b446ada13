"""GPU: listwise_loss_from_batch list by list against the fp64 per-list oracle (tests/_listwise_oracle.py) on every grouping route.

Every case runs the loss forward and backward and asserts
  count and loss   n_valid exact; |loss - ref| <= 1e-5 * max(1, |ref|)
  gradient         for every valid list g:  max_i |d_i - ref_i| <= tol_g * max_i |ref_i|  over the rows of g, rows of invalid lists exactly 0,
                   tol_g = 1e-5 * max(1, max_i |s_i|) + 4 * eps32 * sqrt(n_g / 64)
                   (the project's bound, scaled by the logit magnitude because the rounding of s_i - lse_g is an absolute error of about
                   eps32 * |s| and so a relative error of the softmax; plus a random-walk model, with a margin of 4, of the n_g / 64 sequential
                   fp32 additions of one lane of k_lw_stats)
  reproducibility  the same call twice: bitwise equal loss and gradient
  non-vacuity      on the oracle's own output: enough valid lists, an invalid list of each kind the case is meant to have, |sum_g y| >= 0.25
and prints the worst observed ratio to tol_g (DESIGN.md 5k holds the values measured on an MI355X).  Shapes are the smallest that reach their code:
the route thresholds are GS_MAXB = 8192 rows (one workgroup), 262 144 rows (4096-key tiles), 256 x 4096 rows (the last cooperative size) of
csrc/scan_sort.hip and the grids of k_lw_stats (16 384 lists), k_lw_rank (262 144 lists) and k_lw_norm (524 288 rows) of csrc/listwise.hip."""
import functools

import numpy as np
import pytest
import torch

import dense_ref as R
import _listwise_oracle as LO

pytestmark = pytest.mark.gpu
RTOL = 1e-5
EPS32 = float(np.finfo(np.float32).eps)
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, 2.25, 1e30, -7.0])
SQRT2 = np.float32(1.4142135)


def _mod():
    from rec_now_amd.rec_block import listwise_loss_from_batch as M
    return M


# ---- generators (numpy only: what a case contains depends on its seed alone) ------------------------------------------------------------------
def _assign(rng, B, G, small=48):
    """B rows over G lists of roughly Poisson(B / G) + 1 rows, shuffled, plus `small` single-row lists and `small` lists of two rows (so that
    every kind of invalid list occurs whatever B / G is)."""
    k = np.concatenate([np.arange(G), rng.integers(0, G, B - G)])
    rng.shuffle(k)
    k[:small] = G + np.arange(small)
    k[small:3 * small] = G + small + np.arange(2 * small) // 2
    return k


def _from_sizes(rng, sizes):
    k = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(k)
    return k


def _zipf_sizes(rng, B, G, cap):
    sizes = np.minimum(rng.zipf(1.2, G), cap).astype(np.int64)
    while sizes.sum() > B:                                   # trim the largest
        j = int(sizes.argmax())
        sizes[j] = max(1, sizes[j] - (sizes.sum() - B))
    sizes[int(sizes.argmax())] += B - sizes.sum()
    return sizes


def _labels(rng, k, kind):
    B = k.size
    if kind == 'binary':
        return (rng.random(B) < 0.3).astype(np.float32)
    if kind == 'graded':
        return rng.integers(0, 3, B).astype(np.float32)
    assert kind == 'signed'
    y = np.array([-1.0, 0.0, SQRT2], dtype=np.float32)[rng.integers(0, 3, B)]
    for _ in range(8):                                       # no list with labels but |sum y| < 0.25: one of its -1 becomes 0 (+1 on the sum)
        ysum = np.bincount(k, weights=y.astype(np.float64))
        bad = (np.abs(ysum) < 0.25) & (np.bincount(k, weights=(y != 0)) > 0)
        rows = np.nonzero(bad[k] & (y == -1))[0]
        if rows.size == 0:
            break
        y[rows[np.unique(k[rows], return_index=True)[1]]] = 0.0
    return y


# ---- running and checking ----------------------------------------------------------------------------------------------------------------------
def _dev_ids(ids, dev):
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ids]
    return t[0] if len(t) == 1 else t


def _run(M, dev, ids, y, s, weights=None, do_mask=True, pad_value=-1e9, th=0.5):
    sd = torch.from_numpy(s).to(dev).requires_grad_(True)
    loss, nv = M.listwise_loss_from_batch(_dev_ids(ids, dev), torch.from_numpy(y).to(dev), sd, weights=None if weights is None else torch.from_numpy(weights).to(dev),
                                          do_mask_logits=do_mask, value_of_masked_logit=pad_value, pos_neg_th=th, return_num_list=True)
    loss.backward()
    return loss.detach().cpu().numpy().copy(), int(nv.item()), sd.grad.cpu().numpy().copy()


def _list_tol(ref, s):
    G = ref.valid.size
    smax = np.zeros(G)
    np.maximum.at(smax, ref.row_list, np.abs(s.astype(np.float64)))
    return RTOL * np.maximum(1.0, smax) + 4 * EPS32 * np.sqrt(ref.n_rows / 64.0)


def _check_grad(name, ref, s, d, dref):
    """d against dref list by list; returns the worst ratio of a list's error to its bound."""
    G = ref.valid.size
    d = d.astype(np.float64)
    assert np.isfinite(d).all()
    assert not d[~ref.valid[ref.row_list]].any(), '%s: a row of an invalid list has a gradient' % name
    err, big = np.zeros(G), np.zeros(G)
    np.maximum.at(err, ref.row_list, np.abs(d - dref))
    np.maximum.at(big, ref.row_list, np.abs(dref))
    bound = _list_tol(ref, s) * big
    v = ref.valid & (big > 0)
    ratio = float((err[v] / bound[v]).max()) if v.any() else 0.0
    worst = int(np.nonzero(v)[0][(err[v] / bound[v]).argmax()]) if v.any() else -1
    print('%s: worst per-list gradient error / bound = %.3f (list of %d rows)' % (name, ratio, ref.n_rows[worst] if worst >= 0 else 0))
    assert (err[ref.valid] <= bound[ref.valid]).all(), '%s: %d lists beyond their bound, worst ratio %.3f' % (name, int((err[ref.valid] > bound[ref.valid]).sum()), ratio)
    return ratio


def _check(name, ref, s, loss, nv, d, upstream=1.0):
    print('%s: %d lists, %d valid (kernel %d); loss %.7g ref %.7g' % (name, ref.valid.size, ref.n_valid, nv, float(loss), ref.loss))
    assert nv == ref.n_valid, '%s: %d valid lists, the reference has %d' % (name, nv, ref.n_valid)
    assert abs(float(loss) - ref.loss) <= RTOL * max(1.0, abs(ref.loss))
    return _check_grad(name, ref, s, d, ref.grad * upstream)


def _nonvacuous(ref, min_valid=16, kinds=('nopos', 'noneg', 'single')):
    assert ref.n_valid >= min_valid
    have = {'nopos': (~ref.has_pos & (ref.n_rows > 1)).any(), 'noneg': (ref.has_pos & ~ref.has_neg & (ref.n_rows > 1)).any(),
            'single': ((ref.n_rows == 1) & ~ref.valid).any()}
    for kd in kinds:
        assert have[kd], 'the case has no invalid list of kind %s' % kd
    assert (np.abs(ref.ysum[ref.valid]) >= 0.25).all()


def _case(M, dev, name, ids, y, s, weights=None, do_mask=True, pad_value=-1e9, th=0.5, min_valid=16, kinds=('nopos', 'noneg', 'single'), ref=None):
    """One case end to end; returns (ref, loss, gradient)."""
    if ref is None:
        n_w = None
        if weights is not None:                               # `weights` holds one entry per ROW; the first n_valid of them weigh the valid lists
            n_w = LO.listwise_ref(ids, y, s, None, pad_value if do_mask else 0.0, th).n_valid
        ref = LO.listwise_ref(ids, y, s, None if weights is None else weights[:n_w], pad_value if do_mask else 0.0, th)
    _nonvacuous(ref, min_valid, kinds)
    loss, nv, d = _run(M, dev, ids, y, s, weights, do_mask, pad_value, th)
    _check(name, ref, s, loss, nv, d)
    loss2, nv2, d2 = _run(M, dev, ids, y, s, weights, do_mask, pad_value, th)
    assert nv2 == nv and loss2.tobytes() == loss.tobytes() and d2.tobytes() == d.tobytes(), '%s: two runs differ' % name
    return ref, loss, d


def _weights(rng, B):
    return rng.uniform(0.5, 2.0, B).astype(np.float32)


# ---- the grouping routes -----------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_boundary_zipf_lists_weights(dev):
    """B = 8192 = GS_MAXB: the last size of the one-workgroup grouping; 700 Zipf-sized lists (most of them single rows), weights."""
    rng = np.random.default_rng(101)
    B = 8192
    k = _from_sizes(rng, _zipf_sizes(rng, B, 700, 2048))
    _case(_mod(), dev, 'B8192 zipf', [k.astype(np.float32)], _labels(rng, k, 'binary'), rng.normal(size=B).astype(np.float32), weights=_weights(rng, B))


@functools.lru_cache(maxsize=None)
def _case_8193():
    rng = np.random.default_rng(102)
    B = 8193
    k = _assign(rng, B, 900)
    ids, y, s = [k.astype(np.float32) + np.float32(0.5)], _labels(rng, k, 'graded'), rng.normal(size=B).astype(np.float32)
    return ids, y, s, LO.listwise_ref(ids, y, s, None, 0.0, 0.5)


@functools.lru_cache(maxsize=None)
def _case_20000():
    rng = np.random.default_rng(103)
    B = 20000
    k = _assign(rng, B, 2500)
    ids, y, s = [k.astype(np.float32) * np.float32(0.25)], _labels(rng, k, 'binary'), rng.normal(size=B).astype(np.float32)
    return ids, y, s, LO.listwise_ref(ids, y, s)


def test_first_cooperative_size_fractional_ids_unmasked(dev):
    """B = 8193: the first size of the 2048-key cooperative tile; ids k + 0.5 (no small-integer image), do_mask_logits=False: the
    n_pad * exp(0 - mx) term of the log-sum-exp."""
    ids, y, s, ref = _case_8193()
    _case(_mod(), dev, 'B8193 frac', ids, y, s, do_mask=False, ref=ref)


def test_many_short_lists_stats_grid_stride(dev):
    """B = 40 000 in 25 000 lists of 1 to 3 rows: more lists than the 16 384 waves of k_lw_stats; weights."""
    rng = np.random.default_rng(104)
    B, G = 40000, 25000
    sizes = np.ones(G, dtype=np.int64)
    np.add.at(sizes, rng.permutation(np.repeat(np.arange(G), 2))[:B - G], 1)
    assert sizes.sum() == B and sizes.min() == 1 and sizes.max() == 3
    k = _from_sizes(rng, sizes)
    _case(_mod(), dev, 'B40000 short', [k.astype(np.float32)], _labels(rng, k, 'binary'), rng.normal(size=B).astype(np.float32), weights=_weights(rng, B))


def test_int32_int64_float64_ids_agree_bitwise(dev):
    """B = 20 000, 300 lists: int32 ids (k_group_mid<.., 2>), int64 ids around 2^40 and float64 ids (two key words: recnow_group_keys plus the
    cooperative launch on canonical words).  The same lists, so the three results are equal bit for bit."""
    rng = np.random.default_rng(105)
    B = 20000
    k = _assign(rng, B, 300)
    y, s = _labels(rng, k, 'graded'), rng.normal(size=B).astype(np.float32)
    forms = {'int32': (k - 150).astype(np.int32), 'int64': k.astype(np.int64) * 3 + (1 << 40), 'float64': k.astype(np.float64) + (1 << 40) + 0.25}
    ref = LO.listwise_ref([forms['int32']], y, s)
    out = {}
    for name, ids in forms.items():
        assert np.array_equal(LO.list_index([ids])[0], ref.row_list)
        _, loss, d = _case(_mod(), dev, 'B20000 ' + name, [ids], y, s, ref=ref)
        out[name] = (loss.tobytes(), d.tobytes())
    assert out['int32'] == out['int64'] == out['float64']


@pytest.mark.parametrize('B', [262143, 262144])
def test_4096_key_tile_boundary(dev, B):
    """The last size on 2048-key tiles and the first on 4096-key tiles; 5000 lists, graded labels."""
    rng = np.random.default_rng(106)
    k = _assign(rng, B, 5000)
    _case(_mod(), dev, 'B%d' % B, [k.astype(np.float32)], _labels(rng, k, 'graded'), rng.normal(size=B).astype(np.float32))


def test_last_cooperative_size_rank_and_norm_grid_strides(dev):
    """B = 1 048 576 = 256 x 4096, the last cooperative size, in 400 000 lists: more lists than the 262 144 threads of k_lw_rank and more rows than
    the 524 288 threads of k_lw_norm."""
    rng = np.random.default_rng(107)
    B = 1 << 20
    k = _assign(rng, B, 400000)
    _case(_mod(), dev, 'B1048576', [k.astype(np.float32)], _labels(rng, k, 'binary'), rng.normal(size=B).astype(np.float32))


@pytest.mark.parametrize('form', ['int32', 'float32'])
def test_multi_launch_radix_chain(dev, form):
    """B = 1 048 576 + 2049: 257 tiles of 4096 keys, beyond the co-resident grid: key kernel, radix chain, heads, scans; 3000 lists."""
    rng = np.random.default_rng(108)
    B = (1 << 20) + 2049
    k = _assign(rng, B, 3000)
    ids = (k * 7 - 9000).astype(np.int32) if form == 'int32' else k.astype(np.float32) * np.float32(1.5)
    _case(_mod(), dev, 'B%d %s' % (B, form), [ids], _labels(rng, k, 'binary'), rng.normal(size=B).astype(np.float32))


# ---- numerics ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', ['01', '0.3/0/1.7'])
def test_one_giant_list_beside_short_ones(dev, levels):
    """B = 120 000: one list of 100 000 rows (a single wave's sequential fp32 sums at their longest: 1563 additions per lane) beside 20 000 rows
    in short lists."""
    rng = np.random.default_rng(109)
    B = 120000
    k = np.concatenate([np.zeros(100000, dtype=np.int64), 1 + _assign(rng, 20000, 5000)])
    rng.shuffle(k)
    y = _labels(rng, k, 'binary') if levels == '01' else np.array([0.3, 0.0, 1.7], dtype=np.float32)[rng.integers(0, 3, B)]
    ref, _, _ = _case(_mod(), dev, 'B120000 giant ' + levels, [k.astype(np.float32)], y, rng.normal(size=B).astype(np.float32))
    assert ref.n_rows.max() == 100000 and ref.valid[ref.n_rows.argmax()]


@pytest.mark.parametrize('do_mask', [True, False])
def test_logits_far_from_zero(dev, do_mask):
    """B = 20 000: logits N(0, 1) x 30 (|s| up to about 120); value_of_masked_logit = -50 is a live entry of every row when do_mask_logits."""
    rng = np.random.default_rng(110)
    B = 20000
    k = _assign(rng, B, 600)
    s = (rng.normal(size=B) * 30).astype(np.float32)
    assert np.abs(s).max() > 100
    y = _labels(rng, k, 'binary')
    # a valid list with ONE positive that is also its top logit has a gradient of exp(-gap) all over, below fp32's range at these gaps: the two-row
    # lists are invalid by construction here (labels 0, 0 or 1, 1), and the lists of about 33 rows hold several positives
    two = np.nonzero(k >= 600 + 48)[0]
    y[two] = ((k[two] - 648) % 2).astype(np.float32)
    _case(_mod(), dev, 'B20000 far mask=%s' % do_mask, [k.astype(np.float32)], y, s, do_mask=do_mask, pad_value=-50.0)


@pytest.mark.parametrize('th', [-0.5, 0.0, 1.0])
def test_thresholds(dev, th):
    """B = 5000, labels {-1, 0, sqrt 2}.  th = -0.5: the reference tests `dense_labels > th` on the zero-padded (G, B) row, so every list shorter
    than the batch has a positive -- lists of labels -1 only are valid there."""
    rng = np.random.default_rng(111)
    B = 5000
    k = _assign(rng, B, 1500)
    y = _labels(rng, k, 'signed')
    s = rng.normal(size=B).astype(np.float32)
    ids = [k.astype(np.float32)]
    ref = LO.listwise_ref(ids, y, s, pos_neg_th=th)
    if th < 0:
        member_pos = np.bincount(ref.row_list, weights=(y > np.float32(th))) > 0
        assert (ref.valid & ~member_pos).sum() >= 16        # valid by their padding alone
    _case(_mod(), dev, 'B5000 th=%g' % th, ids, y, s, th=th, kinds=('noneg', 'single') if th < 0 else ('nopos', 'noneg', 'single'), ref=ref)


@pytest.mark.parametrize('B,dtype', [(5000, np.float32), (5000, np.float64), (9000, np.float32), (9000, np.float64)])
def test_special_ids(dev, B, dtype):
    """Ids drawn from [nan, inf, -inf, -0.0, 0.0, -1.5, 2.25, 1e30, -7]: tf.unique makes ONE list of all +inf rows, one of all -inf rows, one of
    -0.0 and +0.0 together, and a list of its own of every NaN row: 7 valid lists.  B = 9000 float32 forms the keys inside the cooperative launch."""
    rng = np.random.default_rng(112)
    pick = rng.integers(0, SPECIAL.size, B)
    ids = [SPECIAL[pick].astype(dtype)]
    y, s = _labels(rng, pick, 'binary'), rng.normal(size=B).astype(np.float32)
    ref = LO.listwise_ref(ids, y, s)
    assert ref.n_valid == 7 and ref.valid.size == 7 + int((pick == 0).sum()) and (ref.n_rows[~ref.valid] == 1).all()
    _case(_mod(), dev, 'B%d special %s' % (B, np.dtype(dtype).name), ids, y, s, min_valid=7, kinds=('single',), ref=ref)


# ---- the other host routes and arguments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['8193', '20000'])
def test_piecewise_route_equals_one_call_route(dev, monkeypatch, which):
    """_ListwiseFused with do_reduce=True (what a list of id tensors or RECNOW_LISTWISE_ONE_CALL=0 selects): equal to the one-call route within
    2e-6 (the bound tests/test_pairwise_gpu.py uses between its two routes) and to the oracle."""
    M = _mod()
    ids, y, s, ref = _case_8193() if which == '8193' else _case_20000()
    do_mask = which != '8193'
    assert M._LW_ONE_CALL
    l1, nv1, d1 = _run(M, dev, ids, y, s, do_mask=do_mask)
    monkeypatch.setattr(M, '_LW_ONE_CALL', False)
    _case(M, dev, 'B%s piecewise' % which, ids, y, s, do_mask=do_mask, ref=ref)
    l0, nv0, d0 = _run(M, dev, ids, y, s, do_mask=do_mask)
    assert nv0 == nv1 == ref.n_valid
    assert abs(float(l0) - float(l1)) <= 2e-6 * max(1.0, abs(float(l1)))
    assert np.abs(d0 - d1).max() <= 2e-6 * np.abs(d1).max()


@pytest.mark.parametrize('B', [8193, 30000])
def test_two_id_tensors(dev, B):
    """[int32, float32]: a list is the set of rows that agree in BOTH tensors."""
    rng = np.random.default_rng(113)
    a, b = rng.integers(0, 40, B).astype(np.int32), rng.integers(0, B // 160, B).astype(np.float32) + np.float32(0.5)
    k = LO.list_index([a.astype(np.int64) * 100000 + b.astype(np.int64)])[0]
    ids = [a, b]
    y, s = _labels(rng, k, 'graded'), rng.normal(size=B).astype(np.float32)
    ref = LO.listwise_ref(ids, y, s)
    assert ref.valid.size > 40 and np.array_equal(ref.row_list, k)
    _case(_mod(), dev, 'B%d two tensors' % B, ids, y, s, ref=ref, kinds=('nopos', 'noneg'))


def test_per_list_losses_and_weight_count(dev):
    """do_reduce=False at B = 20 000 with weights: the per-list losses, the gradient under a random upstream vector, and the ValueError for a
    weight count that is not the number of valid lists."""
    M = _mod()
    ids, y, s, ref0 = _case_20000()
    rng = np.random.default_rng(114)
    w = _weights(rng, ref0.n_valid)
    ref = LO.listwise_ref(ids, y, s, w)
    _nonvacuous(ref)
    gd, yd = _dev_ids(ids, dev), torch.from_numpy(y).to(dev)
    sd = torch.from_numpy(s).to(dev).requires_grad_(True)
    per = M.listwise_loss_from_batch(gd, yd, sd, weights=torch.from_numpy(w).to(dev), do_reduce=False)
    assert per.shape == (ref.n_valid,)
    pv = per.detach().cpu().numpy().astype(np.float64)
    assert (np.abs(pv - ref.per_list) <= RTOL * np.maximum(1.0, np.abs(ref.per_list))).all()
    up = rng.normal(size=ref.n_valid).astype(np.float32)
    (per * torch.from_numpy(up).to(dev)).sum().backward()
    dref = np.where(ref.row_rank >= 0, ref.dbase * up.astype(np.float64)[np.maximum(ref.row_rank, 0)], 0.0)
    _check_grad('B20000 per-list', ref, s, sd.grad.cpu().numpy(), dref)
    for n_w in (ref.n_valid - 1, ref.n_valid + 1):
        with pytest.raises(ValueError, match='one entry per valid list'):
            M.listwise_loss_from_batch(gd, yd, sd.detach(), weights=torch.ones(n_w, device=dev), do_reduce=False)


def test_short_weights_are_zero_padded(dev):
    """do_reduce=True with fewer weights than valid lists: the lists beyond the end weigh 0 (and still count in the mean)."""
    M = _mod()
    ids, y, s, ref0 = _case_20000()
    n_w = ref0.n_valid // 3
    w = _weights(np.random.default_rng(115), n_w)
    ref = LO.listwise_ref(ids, y, s, np.concatenate([w, np.zeros(ref0.n_valid - n_w, dtype=np.float32)]))
    loss, nv, d = _run(M, dev, ids, y, s, weights=w)
    _check('B20000 short weights', ref, s, loss, nv, d)
    assert not d[ref.row_rank >= n_w].any() and np.abs(d[(ref.row_rank >= 0) & (ref.row_rank < n_w)]).max() > 0


def test_plumbing_strided_logits_shapes_label_dtype_upstream(dev):
    """Logits = column 1 of a (B, 3) leaf (what the c5 model passes: its other columns get exactly 0), (B, 1) ids / labels / logits, int64 labels,
    and a non-unit incoming gradient through the one-call route."""
    M = _mod()
    ids, y, s, _ = _case_8193()
    y = (y > 0).astype(np.float32)
    ref = LO.listwise_ref(ids, y, s)
    _nonvacuous(ref)
    rng = np.random.default_rng(116)
    head = rng.normal(size=(s.size, 3)).astype(np.float32)
    head[:, 1] = s
    for shaped in (False, True):
        leaf = torch.from_numpy(head).to(dev).requires_grad_(True)
        gd, yd = torch.from_numpy(ids[0]).to(dev), torch.from_numpy(y.astype(np.int64)).to(dev)
        lg = leaf[:, 1:2] if shaped else leaf[:, 1]
        assert not lg.is_contiguous()
        if shaped:
            gd, yd = gd.reshape(-1, 1), yd.reshape(-1, 1)
        loss, nv = M.listwise_loss_from_batch(gd, yd, lg, return_num_list=True)
        (loss * 2.5).backward()
        g = leaf.grad.cpu().numpy()
        assert not g[:, 0].any() and not g[:, 2].any()
        _check('B8193 plumbing shaped=%s' % shaped, ref, s, loss.detach().cpu().numpy(), int(nv.item()), g[:, 1], upstream=2.5)


def test_dense_outputs_negative_threshold_vs_dense_ref(dev):
    """to_listwise_sample shares k_lw_stats: its dense (G_valid, B) outputs at th = -0.5 against oracle/dense_ref.py, element for element."""
    M = _mod()
    rng = np.random.default_rng(117)
    B = 200
    k = _assign(rng, B, 60, small=0)
    y, s = _labels(rng, k, 'signed'), rng.normal(size=B).astype(np.float32)
    g = k.astype(np.float32)
    rm, rl, rz = R.to_listwise_sample(torch.from_numpy(g), torch.from_numpy(y).double(), torch.from_numpy(s).double(), pos_neg_th=-0.5)
    ref = LO.listwise_ref([g], y, s, pos_neg_th=-0.5)
    member_pos = np.bincount(ref.row_list, weights=(y > -0.5)) > 0
    assert rl.shape[0] == ref.n_valid >= 16 and (ref.valid & ~member_pos).sum() >= 4        # some are valid by their padding alone
    m, lab, lg = M.to_listwise_sample(torch.from_numpy(g).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(s).to(dev), pos_neg_th=-0.5)
    assert np.array_equal(m.cpu().numpy(), rm.numpy())
    # p = y / sum_g y in fp32: the sum of n_g labels carries up to n_g eps32 sum|y|, relative to |sum y| (>= 0.25 by the generator); one more eps32 each for the division and y
    cond = np.bincount(ref.row_list, weights=np.abs(y)) / np.abs(np.where(ref.valid, ref.ysum, 1.0))
    tol = ((ref.n_rows + 2) * EPS32 * cond)[ref.valid]
    assert (np.abs(ref.ysum[ref.valid]) >= 0.25).all()
    assert (np.abs(lab.cpu().numpy() - rl.numpy()) <= tol[:, None] * np.abs(rl.numpy())).all()
    assert np.array_equal(lg.cpu().numpy(), rz.numpy().astype(np.float32))

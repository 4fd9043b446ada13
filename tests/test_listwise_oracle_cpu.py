"""CPU: the per-list fp64 oracle of the listwise loss (tests/_listwise_oracle.py) against oracle/dense_ref.py, which restates the reference's
dense (G, B) formulation line by line and is pinned to its goldens (tests/test_oracle_golden.py).  Valid-list count, per-list losses, loss and
gradient within 1e-12, on seeded random batches of at most 64 rows that cover every kind of id (float32 / float64 / int32 / int64, NaN, +-inf and
signed zeros, two id tensors), the thresholds -0.5 / 0 / 0.5 / 1, masked and unmasked padding and per-list weights."""
import numpy as np
import pytest
import torch

import dense_ref as R
import _listwise_oracle as LO

TOL = 1e-12
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, 2.25, 1e30, -7.0])
KINDS = ('f32', 'f64', 'i32', 'i64', 'special32', 'special64', 'two', 'two_special')
THS = (-0.5, 0.0, 0.5, 1.0)
PADS = ((True, -1e9), (True, -3.0), (False, -1e9))
LABELS = (np.array([-1.0, 0.0, 1.4142135], dtype=np.float32), np.array([0.0, 1.0, 2.0], dtype=np.float32),
          np.array([-1.0, 0.0, 1.0, 2.0], dtype=np.float32))


def _ids(kind, B, rng):
    G = int(rng.integers(1, max(2, B // 2) + 1))
    k = rng.integers(0, G, B)
    if kind == 'f32':
        return [(k.astype(np.float32) * 0.5)]
    if kind == 'f64':
        return [k.astype(np.float64) + 1e-9]                 # no float32 image
    if kind == 'i32':
        return [(k - 3).astype(np.int32)]
    if kind == 'i64':
        return [k.astype(np.int64) + (1 << 40)]
    if kind in ('special32', 'special64'):
        return [SPECIAL[rng.integers(0, SPECIAL.size, B)].astype(np.float32 if kind == 'special32' else np.float64)]
    a = rng.integers(0, 3, B).astype(np.int32)
    b = SPECIAL[rng.integers(0, SPECIAL.size, B)].astype(np.float32) if kind == 'two_special' else rng.integers(0, 4, B).astype(np.float32)
    return [a, b]


def _dense_ids(ids):
    """The ids dense_ref groups by: the tensor itself, or for several tensors one code per distinct TUPLE of python values (tuple equality is
    element-wise python equality: -0.0 == 0.0, inf == inf, and the distinct NaN objects of tolist() equal nothing)."""
    if len(ids) == 1:
        return torch.from_numpy(ids[0])
    seen, code = {}, []
    for t in zip(*[a.tolist() for a in ids]):
        code.append(seen.setdefault(t, len(seen)))
    return torch.tensor(code, dtype=torch.int64)


def _dense(ids, y, s, w_all, do_mask, pad_value, th):
    """dense_ref on the batch: (n_valid, per-list losses, loss, gradient, NaN seen)."""
    s64 = torch.from_numpy(s).double().requires_grad_(True)
    _, rl, rz = R.to_listwise_sample(_dense_ids(ids), torch.from_numpy(y).double(), s64, do_mask_logits=do_mask, value_of_masked_logit=pad_value,
                                     pos_neg_th=th)
    gv = rl.shape[0]
    w = None if w_all is None else torch.from_numpy(w_all[:gv]).double()
    per = R.listwise_loss_via_softmax_cross_entropy_with_logits(rl, rz, w, do_reduce=False)
    loss = R.listwise_loss_via_softmax_cross_entropy_with_logits(rl, rz, w)
    if loss.requires_grad:
        loss.backward()
    grad = s64.grad.numpy() if s64.grad is not None else np.zeros(s.size)
    return gv, per.detach().numpy(), float(loss.detach()), grad, bool(torch.isnan(rl).any())


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    if a.size:
        assert np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def test_oracle_equals_dense_ref_on_random_small_batches():
    kept, drawn_out, seen = 0, 0, set()
    for case in range(288):
        rng = np.random.default_rng(1000 + case)
        kind, th = KINDS[case % len(KINDS)], THS[(case // len(KINDS)) % len(THS)]
        do_mask, pad_value = PADS[(case // 32) % len(PADS)]
        B = int(rng.integers(1, 65))
        ids = _ids(kind, B, rng)
        y = LABELS[case % len(LABELS)][rng.integers(0, LABELS[case % len(LABELS)].size, B)]
        s = rng.normal(size=B).astype(np.float32) * 2
        w_all = rng.uniform(0.5, 2.0, B).astype(np.float32) if rng.random() < 0.5 else None
        gv, per, loss, grad, has_nan = _dense(ids, y, s, w_all, do_mask, pad_value, th)
        if has_nan:                      # a valid list whose labels sum to zero: NaN in the reference, out of scope
            drawn_out += 1
            continue
        ref = LO.listwise_ref(ids, y, s, None if w_all is None else w_all[:gv], pad_value if do_mask else 0.0, th)
        assert ref.n_valid == gv, (case, kind, th)
        _close(ref.per_list, per)
        _close(ref.loss, loss)
        _close(ref.grad, grad)
        kept += 1
        seen.add((kind, th, do_mask, w_all is not None, gv > 0))
    assert kept >= 200 and drawn_out > 0
    for kind in KINDS:
        for th in THS:
            assert any(k == kind and t == th and v for k, t, _, _, v in seen), (kind, th)      # every kind x threshold with valid lists
    assert {(m, w) for _, _, m, w, v in seen if v} == {(True, True), (True, False), (False, True), (False, False)}


def test_oracle_on_the_reference_goldens():
    # reference test_listwise_loss (two valid lists, loss 1.0291535) and test_listwise_loss_case2 (no valid list)
    ids = [np.array([1, 1, 2, 1, 2, 2, 3, 4], dtype=np.float32)]
    y = np.array([1, 1, 1, 0, 0, 0, 1, 0], dtype=np.float32)
    s = np.array([0.1, 0.01, 0.2, 0.001, 0.02, 0.002, 0.3, 0.4], dtype=np.float32)
    ref = LO.listwise_ref(ids, y, s)
    gv, per, loss, grad, _ = _dense(ids, y, s, None, True, -1e9, 0.5)
    assert ref.n_valid == gv == 2 and abs(ref.loss - 1.0291535) < 1e-6
    assert ref.n_rows[ref.valid].mean() == 3.0
    _close(ref.per_list, per)
    _close(ref.loss, loss)
    _close(ref.grad, grad)
    ref = LO.listwise_ref([np.array([3, 4], dtype=np.float32)], np.array([1, 0], dtype=np.float32), np.array([0.3, 0.4], dtype=np.float32))
    assert ref.n_valid == 0 and ref.loss == 0.0 and not ref.grad.any() and ref.per_list.size == 0


def test_oracle_on_the_two_divergences():
    """What tf.unique and the padded (G, B) validity tests make of non-finite ids and of a negative threshold (dense_ref agrees)."""
    ids = [np.array([np.inf, np.inf, -np.inf, -np.inf, np.nan, np.nan, 0.0, -0.0, 7, 7], dtype=np.float32)]
    y = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 1], dtype=np.float32)
    s = np.linspace(-1, 1, 10).astype(np.float32)
    ref = LO.listwise_ref(ids, y, s)
    assert ref.n_valid == _dense(ids, y, s, None, True, -1e9, 0.5)[0] == 3
    assert ref.row_list.tolist() == [0, 0, 1, 1, 2, 3, 4, 4, 5, 5] and ref.valid.tolist() == [True, True, False, False, True, False]
    ids = [np.array([1, 1, 2, 2, 3, 3], dtype=np.float32)]
    y = np.array([-1, -1, 0, -1, 1, -1], dtype=np.float32)
    s = np.linspace(-1, 1, 6).astype(np.float32)
    assert LO.listwise_ref(ids, y, s, pos_neg_th=-0.5).n_valid == _dense(ids, y, s, None, True, -1e9, -0.5)[0] == 3
    y[4] = 2.0                               # (labels 1, -1 sum to zero: NaN in the reference)
    ref = LO.listwise_ref(ids, y, s, pos_neg_th=-0.5)
    gv, per, loss, grad, _ = _dense(ids, y, s, None, True, -1e9, -0.5)
    assert ref.n_valid == gv == 3            # list 1 has no label above -0.5: only the padding of its row makes it one with a positive
    _close(ref.per_list, per)
    _close(ref.grad, grad)
    # ... and a list that fills the batch has no padding
    ref = LO.listwise_ref([np.zeros(3, dtype=np.float32)], np.array([-1, -1, -1], dtype=np.float32), s[:3], pos_neg_th=-0.5)
    assert ref.n_valid == _dense([np.zeros(3, dtype=np.float32)], np.array([-1, -1, -1], dtype=np.float32), s[:3], None, True, -1e9, -0.5)[0] == 0

"""GPU: SparseGNNLayer (csrc/sparse_gnn.hip) against the reference's golden and against the fp64 oracle (tests/_gnn_oracle.py): y, every
layer's output, dx and every weight gradient over a fixed shape list; the callable-activation path; the limits; bit-identical
gradients; the dw reduction over 8192 rows; memory; tensors past 2^31 elements; a state_dict round trip.

Tolerance: max|err| <= 1e-5 * max|oracle| per tensor, as tests/test_star_dense_gpu.py.  A plain fp32 torch evaluation of the same chain
sits at 1e-7 .. 8e-7 of that scale for y, dx and dw (measured on CPU at (B, F, D, L, E) = (4096, 32, 16, 3, 128), (2048, 64, 16, 4, 1024)
and (8192, 16, 8, 8, 240), shared and unshared weights); rn_tanh adds about 2e-7 absolute per layer.  Inputs and gradients are drawn
with a non-zero mean, so that no weight gradient is all cancellation."""
import numpy as np
import pytest
import torch

import _gnn_oracle as G

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def close(a, b, what=''):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if b.size == 0:
        return
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max()
    print('%s: max err %.3g vs scale %.3g (rel %.3g)' % (what, err, scale, err / scale))
    assert err <= RTOL * scale, '%s: max err %.3g vs scale %.3g (rel %.3g)' % (what, err, scale, err / scale)


def graph(kind, F, rng):
    """dict destination -> list of sources."""
    if kind == 'none':
        return {}
    if kind == 'ring':
        return {i: sorted({(i - 1) % F, (i + 1) % F}) for i in range(F)}
    if kind == 'full':                       # E = F^2, self loops included
        return {i: list(range(F)) for i in range(F)}
    if kind == 'complete':                   # E = F (F - 1)
        return {i: [j for j in range(F) if j != i] for i in range(F)}
    # 'rand': node 0 has in-degree F (self loop included), node 1 a self loop only, node F - 1 is isolated (no edge in or out), the rest random
    g = {0: list(range(F - 1)) + ([F - 1] if F < 3 else [])}
    if F > 1:
        g[1] = [1]
    for i in range(2, F - 1):
        n = int(rng.integers(0, min(F - 1, 6) + 1))
        g[i] = sorted(int(v) for v in rng.choice(F - 1, size=n, replace=False))
    return g


def make_layer(F, nbrs, L, share, act, rng, dev, **kw):
    from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer
    layer = SparseGNNLayer(list(range(F)), nbrs, num_layers=L, share_weights_between_layers=share, activation=act, **kw)
    layer._build_device = dev
    layer.build(None)
    E = len(layer.indices)
    indeg = max([len(v) for v in nbrs.values()] + [1])
    scale = min(1.0, 4.0 / indeg)
    vals = {k: ((0.1 + 0.2 * rng.standard_normal(E)) * scale).astype(np.float32) for k in layer.named_weights()}
    layer.set_weights_by_name(vals)
    return layer


def run_case(dev, B, F, D, L, kind, act, share, form, transpose, all_layers=False, grad_layers=None, seed=0):
    rng = np.random.default_rng(seed)
    nbrs = graph(kind, F, rng)
    layer = make_layer(F, nbrs, L, share, act, rng, dev)
    E = len(layer.indices)
    x = (rng.standard_normal((B, F, D)) * 0.5 + 0.3).astype(np.float32)
    # ---- oracle
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w64 = [v.detach().cpu().double().requires_grad_(True) for _, v in sorted(layer.named_weights().items(), key=lambda kv: int(kv[0].split('_')[1]))]
    ref = G.sparse_gnn_bfd(x64, layer.indices, w64, L, act)                       # L x (B, D, F)
    picks = list(range(L)) if all_layers else [L - 1]
    grad_layers = picks if grad_layers is None else grad_layers
    dys = {l: (rng.standard_normal((B, D, F)) + 0.5).astype(np.float32) for l in grad_layers}
    loss = sum((ref[l] * torch.from_numpy(dys[l]).double()).sum() for l in grad_layers)
    rg = torch.autograd.grad(loss, [x64] + w64, allow_unused=True)
    # ---- layer
    xt = torch.from_numpy(x).to(dev)
    if form == 'bfd':
        leaf = xt.clone().requires_grad_(True)
        inp, dx_of = leaf, lambda: leaf.grad
    elif form == '2d':
        leaf = xt.reshape(B, F * D).clone().requires_grad_(True)
        inp, dx_of = leaf, lambda: leaf.grad.reshape(B, F, D)
    elif form == 'bdf':
        leaf = xt.transpose(1, 2).contiguous().requires_grad_(True)
        inp, dx_of = leaf, lambda: leaf.grad.transpose(1, 2)
    elif form == 'list':
        leaves = [xt[:, f, :].contiguous().requires_grad_(True) for f in range(F)]
        inp, dx_of = leaves, lambda: torch.stack([v.grad for v in leaves], 1)
    elif form == 'list_strided':             # non-contiguous views of one (B, F, D) leaf
        leaf = xt.clone().requires_grad_(True)
        inp, dx_of = [leaf[:, f, :] for f in range(F)], lambda: leaf.grad
    else:                                    # 'list_misaligned': contiguous (B, D) views that start 4 bytes past a 16-byte boundary
        leaf = torch.zeros(F * B * D + 1, device=dev)
        leaf[1:] = xt.transpose(0, 1).reshape(-1)
        leaf.requires_grad_(True)
        views = leaf[1:].view(F, B, D)
        assert B == 0 or views[0].data_ptr() % 16 == 4
        inp, dx_of = [views[f] for f in range(F)], lambda: leaf.grad[1:].view(F, B, D).transpose(0, 1)
    out = layer(inp, return_all_layers=all_layers, transpose_outputs=transpose, flattern_outputs=False)
    outs = out if all_layers else [out]
    tag = 'B%d F%d D%d L%d %s E%d %s %s %s %s' % (B, F, D, L, kind, E, act, 'shared' if share else 'unshared', form, 'BFD' if transpose else 'BDF')
    for l, o in zip(picks, outs):
        assert tuple(o.shape) == ((B, F, D) if transpose else (B, D, F))
        close(o.transpose(1, 2) if transpose else o, ref[l], tag + ' y[%d]' % l)
    got = []
    for l in grad_layers:
        o = outs[picks.index(l)]
        dy = torch.from_numpy(dys[l]).to(dev)
        got.append((o * (dy.transpose(1, 2) if transpose else dy)).sum())
    sum(got).backward()
    close(dx_of(), rg[0], tag + ' dx')
    for i, (name, v) in enumerate(sorted(layer.named_weights().items(), key=lambda kv: int(kv[0].split('_')[1]))):
        if E == 0:
            assert v.grad is None or float(v.grad.abs().sum()) == 0.0
        elif rg[1 + i] is None:              # a set no layer with a gradient uses
            assert v.grad is None or float(v.grad.abs().max()) == 0.0
        else:
            close(v.grad, rg[1 + i], tag + ' d' + name)
    return layer


# ---- the reference's golden ----------------------------------------------------------------------------------
def test_reference_golden_all_input_forms(dev, golden):
    # reference tests/layers/test_sparse_gnn_layer.py:19-62
    from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer
    from rec_now_amd.util.numpy_tools import calc_sum_of_abs_diff
    g = golden('sparse_gnn')
    x = torch.from_numpy(g['inputs']).to(dev)
    layer = SparseGNNLayer(fields=[0, 1, 2], field2neighbors={0: [2], 1: [2, 0]}, num_layers=3, share_weights_between_layers=False,
                           activation='tanh')
    for inp in (x, x.reshape(2, -1), [x[:, f, :] for f in range(3)]):
        out = layer(inp, transpose_outputs=False, flattern_outputs=False)
        assert tuple(out.shape) == (2, 4, 3)
        assert calc_sum_of_abs_diff(out, g['golden']) < 1e-5
    flat = layer(x)
    assert tuple(flat.shape) == (2, 12)
    assert torch.equal(flat.reshape(2, 3, 4).transpose(1, 2), layer(x, transpose_outputs=False, flattern_outputs=False))


# ---- the fp64 oracle over the shape list ----------------------------------------------------------------------
#        B     F   D   L  graph       act        share  input form         BFD out
CASES = [
    (7,     2,  1,  1, 'full',     'tanh',    True,  'bfd',             True),
    (7,     2,  5,  3, 'rand',     'relu',    False, 'list',            False),
    (7,     3,  5,  3, 'rand',     'relu',    False, 'list_misaligned', True),
    (1,     17, 8,  8, 'rand',     'sigmoid', False, 'bdf',             True),
    (1,     3,  48, 1, 'ring',     'linear',  True,  'bdf',             False),
    (7,     17, 16, 3, 'none',     'sigmoid', True,  '2d',              True),
    (7,     32, 8,  1, 'rand',     'relu',    True,  'list_strided',    True),
    (7,     64, 5,  8, 'rand',     'tanh',    False, 'bfd',             False),
    (7,     64, 48, 8, 'complete', 'tanh',    True,  'list',            True),
    (1000,  32, 16, 3, 'ring',     'tanh',    False, '2d',              True),
    (1000,  64, 48, 3, 'full',     'linear',  True,  'bfd',             True),
    (1000,  17, 1,  3, 'rand',     'sigmoid', False, 'list',            False),
    (1000,  3,  5,  8, 'full',     'tanh',    True,  'bdf',             False),
    (1000,  32, 48, 3, 'complete', 'tanh',    False, 'bdf',             True),
    (8192,  32, 16, 3, 'rand',     'tanh',    False, 'list',            True),
    (8192,  17, 8,  1, 'full',     'sigmoid', True,  'bfd',             False),
    (8192,  2,  1,  8, 'ring',     'linear',  False, 'bdf',             True),
    (7,     3,  100, 2, 'rand',    'tanh',    False, 'bfd',             True),      # D > 64: channel tiles of one row
    (7,     3,  67, 2, 'rand',     'tanh',    False, 'bdf',             False),
]


@pytest.mark.parametrize('B,F,D,L,kind,act,share,form,transpose', CASES)
def test_against_oracle(dev, B, F, D, L, kind, act, share, form, transpose):
    run_case(dev, B, F, D, L, kind, act, share, form, transpose)


@pytest.mark.parametrize('B,F,D,L,kind,act,share,form,transpose,grad_layers', [
    (7,    3,  5,  3, 'rand', 'tanh',    False, 'bfd',  True,  None),
    (1000, 32, 16, 3, 'ring', 'tanh',    True,  'list', False, [0, 2]),
    (7,    64, 8,  8, 'rand', 'sigmoid', False, 'bdf',  True,  [1, 4, 7]),
    (1000, 17, 5,  8, 'rand', 'relu',    True,  '2d',   True,  [0, 3]),           # the last layer's output gets no gradient
    (7,    2,  1,  1, 'full', 'linear',  True,  'bfd',  False, None),
])
def test_all_layers_and_gradients_into_several(dev, B, F, D, L, kind, act, share, form, transpose, grad_layers):
    run_case(dev, B, F, D, L, kind, act, share, form, transpose, all_layers=True, grad_layers=grad_layers)


def test_empty_batch(dev):
    run_case(dev, 0, 3, 4, 2, 'rand', 'tanh', False, 'bfd', True)


@pytest.mark.parametrize('act', [torch.tanh, lambda t: t * torch.sigmoid(t)])
def test_callable_activation(dev, act):
    fn64 = act
    run_case(dev, 7, 5, 8, 3, 'rand', fn64, False, 'bfd', True)
    run_case(dev, 7, 5, 8, 3, 'ring', fn64, True, 'list', False, all_layers=True, grad_layers=[0, 2])


def test_limits(dev):
    from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer
    layer = SparseGNNLayer(list(range(65)), {0: [1]})
    with pytest.raises(NotImplementedError, match='at most 64'):
        layer(torch.zeros(2, 65, 4, device=dev))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        SparseGNNLayer([0, 1, 2], {0: [1]})(torch.zeros(2, 3, 4))


def test_frozen_weights_and_constant_input(dev):
    rng = np.random.default_rng(5)
    nbrs = graph('rand', 6, rng)
    frozen = make_layer(6, nbrs, 2, False, 'tanh', rng, dev, trainable=False)
    x = torch.randn(9, 6, 4, device=dev, requires_grad=True)
    frozen(x).sum().backward()
    assert x.grad is not None and all(v.grad is None for v in frozen.named_weights().values())
    live = make_layer(6, nbrs, 2, False, 'tanh', rng, dev)
    live(torch.randn(9, 6, 4, device=dev)).sum().backward()                      # the input needs no gradient
    assert all(v.grad is not None for v in live.named_weights().values())


def _grads(layer, x, dy):
    x.grad = None
    layer.zero_grad(set_to_none=True)
    layer(x).backward(dy)
    return [x.grad.clone()] + [v.grad.clone() for v in layer.named_weights().values()]


def test_gradients_bit_identical_over_runs(dev):
    rng = np.random.default_rng(7)
    layer = make_layer(32, graph('rand', 32, rng), 3, True, 'tanh', rng, dev)
    x = (torch.randn(8192, 32, 16, device=dev) * 0.5 + 0.3).requires_grad_(True)
    dy = torch.randn(8192, 32 * 16, device=dev) + 0.5
    first = _grads(layer, x, dy)
    for _ in range(3):
        for a, b in zip(first, _grads(layer, x, dy)):
            assert torch.equal(a, b)


def test_dw_of_8192_rows_checks_the_workspace_reduction(dev):
    """8192 rows of D = 16 are 2048 tiles on 1024 workgroups: every workspace row holds two tiles' sums, and the reduction adds 1024 rows."""
    run_case(dev, 8192, 32, 16, 3, 'ring', 'tanh', True, 'bfd', True, seed=11)


def test_memory(dev):
    from rec_now_amd import _lib
    B, F, D, L = 65536, 32, 32, 3
    rng = np.random.default_rng(9)
    layer = make_layer(F, graph('ring', F, rng), L, False, 'tanh', rng, dev)
    x = (torch.randn(B, F, D, device=dev) * 0.5).requires_grad_(True)
    dy = torch.randn(B, F * D, device=dev)
    layer(x[:4])
    torch.cuda.synchronize()
    out_bytes = B * F * D * 4
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = layer(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise <= out_bytes + (1 << 20), 'forward rise %.1f MB' % (rise / 2 ** 20)
    ws = _lib.load().recnow_sparse_gnn_workspace_bytes(B, F, D, 2 * F, L)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y.backward(dy)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise <= out_bytes + ws + (1 << 20), 'backward rise %.1f MB (dx %.1f MB, workspace %.1f MB)' % (rise / 2 ** 20, out_bytes / 2 ** 20, ws / 2 ** 20)


def test_past_two_to_the_31_elements(dev):
    """B F D > 2^31: forward and dx on the first rows, the last rows and the rows on each side of the 2^31-element boundary.  Rows are
    independent, so the oracle on those rows alone is exact."""
    F, D, L = 32, 32, 2
    edge = (1 << 31) // (F * D)
    B = edge + 70
    rng = np.random.default_rng(13)
    layer = make_layer(F, graph('rand', F, rng), L, False, 'tanh', rng, dev)
    x = torch.empty(B, F, D, device=dev)
    for s in range(0, B, 1 << 18):
        x[s:s + (1 << 18)].normal_(0.3, 0.5)
    x.requires_grad_(True)
    assert x.numel() > 1 << 31
    y = layer(x, flattern_outputs=False)
    rows = torch.tensor(list(range(4)) + list(range(edge - 3, edge + 3)) + list(range(B - 4, B)), device=dev)
    dy_rows = (torch.randn(len(rows), F, D, device=dev) + 0.5)
    dy = torch.zeros_like(y)
    dy[rows] = dy_rows
    y.backward(dy)
    x64 = x.detach()[rows].cpu().double().requires_grad_(True)
    w64 = [v.detach().cpu().double() for _, v in sorted(layer.named_weights().items(), key=lambda kv: int(kv[0].split('_')[1]))]
    ref = G.sparse_gnn_bfd(x64, layer.indices, w64, L, 'tanh')[-1]
    close(y.detach()[rows].transpose(1, 2), ref, 'y rows')
    (ref * dy_rows.cpu().double().transpose(1, 2)).sum().backward()
    close(x.grad[rows], x64.grad, 'dx rows')
    untouched = torch.tensor([5, edge - 10, edge + 10, B - 9], device=dev)
    assert float(x.grad[untouched].abs().max()) == 0.0                            # a zero output gradient gives a zero input gradient


def test_state_dict_round_trip(dev):
    rng = np.random.default_rng(17)
    nbrs = graph('rand', 9, rng)
    a = make_layer(9, nbrs, 3, False, 'tanh', rng, dev)
    b = make_layer(9, nbrs, 3, False, 'tanh', rng, dev)
    x = torch.randn(33, 9, 6, device=dev)
    assert not torch.equal(a(x), b(x))
    b.load_state_dict(a.state_dict())
    assert torch.equal(a(x), b(x))
    for k, v in a.named_weights().items():
        assert torch.equal(v, b.named_weights()[k])

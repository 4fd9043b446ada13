"""GPU parity of attention_by_dnn (csrc/attention_dnn.hip): the reference's golden, then forward and every gradient against the
fp64 oracle (tests/_din_oracle.py, run in fp64 on the device) over a list of shapes, the optional upstream gradients, empty and
non-contiguous / fp64 inputs, model reuse, run-to-run bit identity, the memory footprint and 64-bit row offsets."""
import numpy as np
import pytest
import torch

import _din_oracle as O
from rec_now_amd.rec_block.attention import attention_by_dnn
from rec_now_amd.util.numpy_tools import calc_sum_of_abs_diff

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def close(a, b, rtol=RTOL, scale=None):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    s = max(np.abs(b).max() if scale is None and b.size else (scale or 0.0), 1e-30)
    err = np.abs(a - b).max() if b.size else 0.0
    assert err <= rtol * s, 'max err %.3g vs scale %.3g' % (err, s)


def _weights(model):
    nl = len(model.dnn_dims)
    w = model.named_weights()
    return [w['layer%d/kernel' % i] for i in range(nl)], [w['layer%d/bias' % i] for i in range(nl)]


def _randomise(model, gen):
    """glorot weights with non-zero biases (the default zeros would leave the bias paths untested)."""
    ks, bs = _weights(model)
    with torch.no_grad():
        for b in bs:
            b.copy_(torch.randn(b.shape, generator=gen) * 0.2)


def _check(model, user, doc, act, dmat=True, dsum=True, gen=None):
    """forward + backward of the fused model against the fp64 oracle with the same weights."""
    u = user.detach().clone().requires_grad_(True)
    d = doc.detach().clone().requires_grad_(True)
    mat, ssum = model(u, d)
    B, L, D = user.shape
    gm = torch.randn((B, D), generator=gen).to(user.device)
    gs = torch.randn((B, 1), generator=gen).to(user.device)
    loss = 0.0
    if dmat:
        loss = loss + (mat * gm).sum()
    if dsum:
        loss = loss + (ssum * gs).sum()
    ks, bs = _weights(model)
    for p in ks + bs:
        p.grad = None
    loss.backward()
    u64 = user.detach().double().requires_grad_(True)
    d64 = doc.detach().double().requires_grad_(True)
    k64 = [k.detach().double().requires_grad_(True) for k in ks]
    b64 = [b.detach().double().requires_grad_(True) for b in bs]
    rmat, rsum = O.attention_by_dnn(u64, d64, k64, b64, act)
    rloss = 0.0
    if dmat:
        rloss = rloss + (rmat * gm.double()).sum()
    if dsum:
        rloss = rloss + (rsum * gs.double()).sum()
    rloss.backward()
    close(mat, rmat)
    close(ssum, rsum)
    close(u.grad, u64.grad)
    close(d.grad, d64.grad)
    for i, (k, b, rk, rb) in enumerate(zip(ks, bs, k64, b64)):
        close(k.grad, rk.grad)
        close(b.grad, rb.grad, scale=max(float(rb.grad.abs().max()), float(rk.grad.abs().max())))


def test_reference_golden(dev, golden):
    # /root/reference/tests/rec_block/test_attention.py:57-76, with the TFSeededRNG(0) kernels of tests/golden/make_golden_din.py
    g = golden('attention_dnn')
    user, doc = torch.from_numpy(g['user']).to(dev), torch.from_numpy(g['doc']).to(dev)
    mat, ssum, model = attention_by_dnn(user, doc, dnn_dims=[32, 24, 1])
    assert mat.shape == (2, 2) and ssum.shape == (2, 1) and model.name == 'din'
    nl = len(g['dims'])
    model.set_weights_by_name({**{'layer%d/kernel' % i: g['kernel%d' % i] for i in range(nl)},
                               **{'layer%d/bias' % i: g['bias%d' % i] for i in range(nl)}})
    mat, ssum = model(user, doc)
    assert calc_sum_of_abs_diff(mat, g['golden_mat']) < 1e-5
    assert calc_sum_of_abs_diff(ssum, g['golden_sum']) < 1e-5


# Every value of B {1, 7, 513, 4096}, L {1, 2, 17, 50, 300}, D {2, 3, 16, 64, 256}, the five dims and the four activations at least
# once.  Tiles are 32 positions: L 300 / 50 / 17 rows span several tiles and tiles end inside rows; L 1 / 2 put many rows in a tile.
CASES = [
    (1, 1, 2, [1], 'relu'),
    (7, 17, 3, [32, 24, 1], 'tanh'),
    (513, 50, 16, [80, 40], 'sigmoid'),
    (4096, 2, 64, [200, 80, 1], 'relu'),
    (7, 300, 256, [256, 256, 256], 'linear'),
    (513, 17, 64, [200, 80, 1], 'tanh'),
    (1, 300, 16, [1], 'sigmoid'),
    (4096, 50, 2, [32, 24, 1], 'linear'),
    (513, 1, 256, [80, 40], 'relu'),
    (7, 2, 3, [256, 256, 256], 'sigmoid'),
]


@pytest.mark.parametrize('B,L,D,dims,act', CASES, ids=['B%d-L%d-D%d-%s-%s' % (c[0], c[1], c[2], 'x'.join(map(str, c[3])), c[4]) for c in CASES])
def test_forward_backward_vs_oracle(dev, B, L, D, dims, act):
    gen = torch.Generator().manual_seed(B * 1000 + L * 10 + D)
    user = (torch.rand((B, L, D), generator=gen) * 2 - 1).to(dev)
    doc = (torch.rand((B, D), generator=gen) * 2 - 1).to(dev)
    dims = list(dims)
    _, _, model = attention_by_dnn(user[:1], doc[:1], dims, dnn_activation=act)
    assert dims[-1] == 1
    _randomise(model, gen)
    _check(model, user, doc, act, gen=gen)


@pytest.mark.parametrize('which', ['dmat', 'dsum'])
def test_one_output_gradient(dev, which):
    gen = torch.Generator().manual_seed(5)
    user = torch.randn((33, 40, 16), generator=gen).to(dev)
    doc = torch.randn((33, 16), generator=gen).to(dev)
    _, _, model = attention_by_dnn(user, doc, [48, 24], dnn_activation='tanh')
    _randomise(model, gen)
    _check(model, user, doc, 'tanh', dmat=which == 'dmat', dsum=which == 'dsum', gen=gen)


@pytest.mark.parametrize('B,L', [(0, 5), (6, 0), (0, 0)])
def test_empty(dev, B, L):
    D = 8
    user = torch.randn((B, L, D), device=dev, requires_grad=True)
    doc = torch.randn((B, D), device=dev, requires_grad=True)
    mat, ssum, model = attention_by_dnn(user, doc, [16])
    assert mat.shape == (B, D) and ssum.shape == (B, 1)
    assert float(mat.detach().abs().sum()) == 0.0 and float(ssum.detach().abs().sum()) == 0.0
    (mat.sum() + ssum.sum()).backward()
    assert user.grad.shape == user.shape and doc.grad.shape == doc.shape
    assert float(doc.grad.abs().sum()) == 0.0
    for p in model.named_weights().values():
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0


def test_noncontiguous_and_fp64(dev):
    gen = torch.Generator().manual_seed(11)
    B, L, D = 45, 19, 12
    base = torch.randn((L, B, 2 * D), generator=gen).to(dev)
    user = base.transpose(0, 1)[:, :, ::2]                # (B, L, D), no unit stride anywhere
    doc = torch.randn((D, B), generator=gen).to(dev).t()
    assert not user.is_contiguous() and not doc.is_contiguous()
    _, _, model = attention_by_dnn(user, doc, [24, 1])
    _randomise(model, gen)
    _check(model, user, doc, 'relu', gen=gen)
    u64 = user.double().requires_grad_(True)
    d64 = doc.double().requires_grad_(True)
    mat, ssum = model(u64, d64)
    (mat.sum() + ssum.sum()).backward()
    assert u64.grad.dtype == torch.float64 and d64.grad.dtype == torch.float64
    ks, bs = _weights(model)
    rmat, rsum = O.attention_by_dnn(u64.detach(), d64.detach(), [k.detach().double() for k in ks], [b.detach().double() for b in bs])
    close(mat, rmat)
    close(ssum, rsum)


def test_model_reuse(dev):
    gen = torch.Generator().manual_seed(3)
    u1, d1 = torch.randn((20, 9, 16), generator=gen).to(dev), torch.randn((20, 16), generator=gen).to(dev)
    u2, d2 = torch.randn((70, 33, 16), generator=gen).to(dev), torch.randn((70, 16), generator=gen).to(dev)
    mat1, _, model = attention_by_dnn(u1, d1, [32, 16], dnn_activation='sigmoid')
    ks, bs = _weights(model)
    rmat1, _ = O.attention_by_dnn(u1.double(), d1.double(), [k.detach().double() for k in ks], [b.detach().double() for b in bs], 'sigmoid')
    close(mat1, rmat1)
    _randomise(model, gen)
    _check(model, u2, d2, 'sigmoid', gen=gen)
    n_params = len(list(model.parameters()))
    model(u1, d1)
    assert len(list(model.parameters())) == n_params == 6


def test_backward_bit_identical(dev):
    gen = torch.Generator().manual_seed(9)
    user = torch.randn((3000, 37, 64), generator=gen).to(dev)
    doc = torch.randn((3000, 64), generator=gen).to(dev)
    _, _, model = attention_by_dnn(user[:1], doc[:1], [200, 80, 1])
    _randomise(model, gen)
    gm = torch.randn((3000, 64), generator=gen).to(dev)
    runs = []
    for _ in range(2):
        u = user.clone().requires_grad_(True)
        d = doc.clone().requires_grad_(True)
        for p in model.parameters():
            p.grad = None
        mat, ssum = model(u, d)
        ((mat * gm).sum() + ssum.sum()).backward()
        runs.append([u.grad, d.grad] + [p.grad.clone() for p in model.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_memory_far_below_one_activation(dev):
    B, L, D, H1 = 16384, 64, 16, 256
    act_bytes = B * L * H1 * 4
    assert act_bytes >= 1 << 30
    gen = torch.Generator().manual_seed(1)
    user = (torch.rand((B, L, D), generator=gen) - 0.5).to(dev).requires_grad_(True)
    doc = (torch.rand((B, D), generator=gen) - 0.5).to(dev).requires_grad_(True)
    _, _, model = attention_by_dnn(user[:1], doc[:1], [H1, 1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    mat, ssum = model(user, doc)
    (mat.sum() + ssum.sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    # what must exist: duser (B L D) and the small outputs; everything else is the bounded workspace
    assert peak < act_bytes / 4, 'peak %.0f MB over the inputs, one (B, L, H1) activation is %.0f MB' % (peak / 2**20, act_bytes / 2**20)


def test_user_past_2_pow_31_elements(dev):
    B, L, D = 131072, 257, 64                        # 2.16e9 elements: rows near the end sit past 2^31 floats
    assert B * L * D > 2 ** 31
    user = torch.empty((B, L, D), device=dev)
    user.uniform_(-1, 1, generator=torch.Generator(device=dev).manual_seed(0))
    doc = torch.rand((B, D), device=dev) - 0.5
    user.requires_grad_(True)
    _, _, model = attention_by_dnn(user[:1].detach(), doc[:1], [8, 1])
    _randomise(model, torch.Generator().manual_seed(2))
    mat, ssum = model(user, doc)
    gm = torch.randn((B, D), device=dev)
    (mat * gm).sum().backward()
    sl = slice(B - 3, B)
    ks, bs = _weights(model)
    u64 = user.detach()[sl].double().requires_grad_(True)
    rmat, rsum = O.attention_by_dnn(u64, doc[sl].double(), [k.detach().double() for k in ks], [b.detach().double() for b in bs])
    (rmat * gm[sl].double()).sum().backward()
    close(mat[sl], rmat)
    close(ssum[sl], rsum)
    close(user.grad[sl], u64.grad)

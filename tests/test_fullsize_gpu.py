"""GPU parity at BASELINE.json's full sizes.  The interaction layers are row-independent, so a full-size run is checked
(a) on a random subset of rows, forward output and input gradient, against the oracle evaluated on just those rows with the
same weights (fp64 autograd of the dense restatement), and (b) through the linearity of the weight gradients in the batch:
dW(all rows) = dW(first half) + dW(second half).  Tolerance 1e-5 relative (north_star)."""
import os

import numpy as np
import pytest
import torch

import dense_ref as R

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def close(a, b, rtol=RTOL, scale=None):
    a = a.detach().cpu().double().numpy() if hasattr(a, 'detach') else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if hasattr(b, 'detach') else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    s = max(np.abs(b).max() if scale is None else scale, 1e-30)
    err = np.abs(a - b).max()
    if os.environ.get('RECNOW_TEST_MARGIN_LOG') and err > 0.3 * rtol * s:      # diagnostics: comparisons that use more than 30 % of their bound
        with open(os.environ['RECNOW_TEST_MARGIN_LOG'], 'a') as fh:
            fh.write('%.3f of the bound  %s  %s\n' % (err / (rtol * s), os.environ.get('PYTEST_CURRENT_TEST', ''), ''))
    assert err <= rtol * s, 'max err %.3g vs scale %.3g (rel %.3g)' % (err, s, err / s)


def _weight_grads(layer):
    return {k: p.grad.clone() for k, p in layer.named_weights().items() if p.grad is not None}


def _zero(layer):
    for p in layer.parameters():
        p.grad = None


def test_dcn_mix_config3_full_size(dev):
    """configs[2]: B = 65536, D = 64 x 16, S = 64, N = 2, L = 3 (the north-star layer, exact-128 path)."""
    from rec_now_amd.layers.dcn_mix_layer import DCNMixLayer
    B, D, S, N, L = 65536, 1024, 64, 2, 3
    g = torch.Generator(device='cpu').manual_seed(11)
    x = torch.randn(B, D, generator=g) * 0.5
    gy = torch.randn(B, D, generator=g)
    layer = DCNMixLayer(S, num_layer=L, num_expert=N)
    xd = x.to(dev).requires_grad_(True)
    layer(xd[:256])
    y = layer(xd)
    y.backward(gy.to(dev))
    full = _weight_grads(layer)
    rows = torch.from_numpy(np.random.default_rng(1).choice(B, 192, replace=False))
    w64 = {k: p.detach().cpu().double().requires_grad_(True) for k, p in layer.named_weights().items()}
    pick = lambda fmt: [w64[fmt % l] for l in range(L)]     # noqa: E731
    x64 = x[rows].double().requires_grad_(True)
    ry = R.dcn_mix_layer(x64, pick('origin_to_sub_kernels_of_layer%d'), pick('sub_to_sub_kernels_of_layer%d'),
                         pick('sub_to_origin_kernels_of_layer%d'), pick('bias_of_layer%d'), pick('gate_of_layer%d/kernel'), 'tanh', 'tanh')
    ry.backward(gy[rows].double())
    close(y[rows.to(dev)], ry)
    close(xd.grad[rows.to(dev)], x64.grad)
    # linearity of the weight gradients in the batch
    halves = []
    for lo, hi in ((0, B // 2), (B // 2, B)):
        _zero(layer)
        xh = x[lo:hi].to(dev)
        layer(xh).backward(gy[lo:hi].to(dev))
        halves.append(_weight_grads(layer))
    for k in full:
        close(halves[0][k] + halves[1][k], full[k], rtol=3e-5)


def test_cin_config4_per_rank_size(dev):
    """configs[3] layer alone: F = 64, D = 16, H = [128, 128, 128]: the output, d / d x on ALL rows and ALL THREE
    weight gradients against the fp64 oracle evaluated chunk-wise over the whole batch (oracle/dense_ref.cin_layer_gemm_form,
    reference /root/reference/rec_now/layers/cin_layer.py:101-110; weight gradients summed over the chunks in fp64).
    B = 2048 here; the per-rank size B = 16 384 of the same layer -- all rows, all weight gradients -- runs inside the c4 MODEL test
    (tests/test_models_gpu.py::test_config4_model_per_rank_size_vs_oracle): one fp64 oracle of that size per suite run."""
    from _chunked_oracle import run_chunked
    from rec_now_amd.layers.cin_layer import CINLayer
    B, F, D, Hs = 2048, 64, 16, [128, 128, 128]
    g = torch.Generator(device='cpu').manual_seed(12)
    x = torch.randn(B, F * D, generator=g) * 0.3
    gy = torch.randn(B, D, generator=g)
    layer = CINLayer(Hs)
    xd = [x[:, f * D:(f + 1) * D].contiguous().to(dev).requires_grad_(True) for f in range(F)]
    y = layer(xd)
    y.backward(gy.to(dev))
    w64 = {k: layer.idx2weight[k].detach().cpu().double().requires_grad_(True) for k in range(1, len(Hs) + 1)}
    fwd = lambda xc: R.cin_layer_gemm_form(xc, [w64[k] for k in range(1, len(Hs) + 1)], F, D, True, True)      # noqa: E731
    (ry,), rdx, rgrads = run_chunked(fwd, x, gy, w64, chunk=512)
    close(y, ry)
    close(torch.cat([a.grad for a in xd], dim=1), rdx)
    for k in range(1, len(Hs) + 1):
        close(layer.idx2weight[k].grad, rgrads[k])


def test_fm_config4_full_size(dev):
    """configs[3]: FMLayer at the global batch B = 131072, F = 64, D = 16 -- the whole batch against the oracle."""
    from rec_now_amd.layers.fm_layer import FMLayer
    B, F, D = 131072, 64, 16
    g = torch.Generator(device='cpu').manual_seed(13)
    xs = [torch.rand(B, D, generator=g) - 0.5 for _ in range(F)]
    gy = torch.randn(B, 1, generator=g)
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    y = FMLayer()(xd)
    y.backward(gy.to(dev))
    x64 = [x.double().requires_grad_(True) for x in xs]
    ry = R.fm_layer(x64)
    ry.backward(gy.double())
    st = torch.stack(xs).double()
    scale = float((0.5 * ((st.sum(0) ** 2).sum(1) + (st ** 2).sum((0, 2)))).max())     # magnitude of the subtracted terms
    close(y, ry, scale=scale)
    gs = max(float(v.grad.abs().max()) for v in x64)
    for a, b in zip(xd[::9], x64[::9]):
        close(a.grad, b.grad, scale=gs)


@pytest.mark.parametrize('B,F,D', [(131072 + 37, 6, 16), (65536 + 3, 9, 32)])
def test_fm_wide_kernels_ragged_sizes(dev, B, F, D):
    """The four-chunks-per-thread FM kernels (csrc/fm.hip k_fm_fwd_wide / k_fm_bwd_wide: from 524 288 float4 chunks on) on batches
    that are not a multiple of their 1024-chunk step (the forward masks the tail, the backward takes the one-chunk kernel) and a
    field count that is not a multiple of the four fields in flight."""
    from rec_now_amd.layers.fm_layer import FMLayer
    g = torch.Generator(device='cpu').manual_seed(B)
    xs = [torch.rand(B, D, generator=g) - 0.5 for _ in range(F)]
    gy = torch.randn(B, 1, generator=g)
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    y = FMLayer()(xd)
    y.backward(gy.to(dev))
    x64 = [x.double().requires_grad_(True) for x in xs]
    ry = R.fm_layer(x64)
    ry.backward(gy.double())
    st = torch.stack(xs).double()
    scale = float((0.5 * ((st.sum(0) ** 2).sum(1) + (st ** 2).sum((0, 2)))).max())
    close(y, ry, scale=scale)
    gs = max(float(v.grad.abs().max()) for v in x64)
    for a, b in zip(xd, x64):
        close(a.grad, b.grad, scale=gs)


def test_ple_config5_per_rank_size(dev):
    """configs[4] per-rank share: B = 32768, D_in = 128 x 32, 3 tasks.  Rows are independent, so the 512-row subset is held to the fp64 oracle
    (oracle/dense_ref.ple_layer on the layer's own weights, tests/_ple_oracle.oracle_layers): the full-batch outputs and input gradient of those
    rows, per row, within 1e-5 x the row's max |ref|.  Then the size-independent checks: row independence on the GPU (the outputs and input
    gradients of a row do not depend on which batch it is evaluated in) and linearity of the weight gradients."""
    from rec_now_amd.layers.ple_layer import PLELayer
    B, Din = 32768, 4096
    g = torch.Generator(device='cpu').manual_seed(14)
    x = torch.randn(B, Din, generator=g) * 0.05
    # tanh, not relu: at a relu kink a pre-activation of ~1e-9 flips sign with the summation order (split-K or not), and one
    # flipped mask element moves a weight-gradient entry by O(1/sqrt(B)) -- a property of fp32, not of the kernels
    layer = PLELayer(3, [[512, 256], [256, 128]], 2, 1, activation='tanh')
    xd = x.to(dev).requires_grad_(True)
    outs = layer(xd)
    gys = [torch.randn(B, o.shape[1], generator=g) for o in outs]
    sum((o * gy.to(dev)).sum() for o, gy in zip(outs, gys)).backward()
    full = _weight_grads(layer)
    sub = slice(4096, 4096 + 512)
    _zero(layer)
    xs = x[sub].to(dev).requires_grad_(True)
    souts = layer(xs)
    sum((o * gy[sub].to(dev)).sum() for o, gy in zip(souts, gys)).backward()
    from _ple_oracle import oracle_layers, row_margin, torch_np
    layers64, _ = oracle_layers(layer)
    x64 = x[sub].double().requires_grad_(True)
    routs = R.ple_layer(x64, layers64, layer.is_shared_tasks, activation='tanh')
    sum((o * gy[sub].double()).sum() for o, gy in zip(routs, gys)).backward()
    for t, (o, ro) in enumerate(zip(outs, routs)):
        close(o[sub], ro)
        m = row_margin(torch_np(ro), torch_np(o[sub]), RTOL)
        print('ple config5: output %d of the full batch vs the fp64 oracle on rows 4096..4607: worst per-row margin %.3f of the bound' % (t, m))
        assert m <= 1.0, (t, m)
    close(xd.grad[sub], x64.grad)
    m = row_margin(torch_np(x64.grad), torch_np(xd.grad[sub]), RTOL)
    print('ple config5: dx of the full batch vs the fp64 oracle: worst per-row margin %.3f of the bound' % m)
    assert m <= 1.0, m
    for o, so in zip(outs, souts):
        close(so, o[sub], rtol=5e-6)           # different batch sizes take different tile paths (summation order); tanh via exp2 / rcp
    close(xs.grad, xd.grad[sub], rtol=5e-6)
    halves = []
    for lo, hi in ((0, B // 2), (B // 2, B)):
        _zero(layer)
        ho = layer(x[lo:hi].to(dev))
        sum((o * gy[lo:hi].to(dev)).sum() for o, gy in zip(ho, gys)).backward()
        halves.append(_weight_grads(layer))
    for k in full:
        close(halves[0][k] + halves[1][k], full[k], rtol=3e-5)

"""GPU: kernels that own more than 64 KiB of dynamic LDS, run in ONE process on cuda:0 and then on cuda:1.

The limit of a kernel's dynamic LDS is an attribute of the function on the current device, so rn_lds_grant (csrc/lds_grant.hip) raises it per
(kernel, device).  Whether this runtime refuses a launch on a device whose limit was never raised is not known: the test documents the rule (a second
device computes what the first does) and does not prove that per-process flags failed.  Two cases, each from the same CPU-generated inputs:
attention_by_dnn forward and backward at D = 256 with hidden widths (256,), whose plan needs 66 432 bytes, the smallest shape above 64 KiB; and the
AFMLayer backward at F = 64, D = 64, A = 4, which needs 75 136 bytes.  The two devices must agree bit for bit, and each must match the layer's fp64
oracle within the bound of the layer's own GPU test (test_attention_dnn_gpu.close, test_afm_layer_gpu._hold_all).
Skips when fewer than two devices are visible."""
import pytest
import torch

import _din_oracle as DO
import test_afm_layer_gpu as TA
import test_attention_dnn_gpu as TD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def devices(dev):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    return [torch.device('cuda:0'), torch.device('cuda:1')]


def test_attention_by_dnn_on_a_second_device(devices):
    from rec_now_amd.rec_block.attention import attention_by_dnn
    gen = torch.Generator().manual_seed(256)
    B, L, D, act = 5, 7, 256, 'tanh'
    user, doc = torch.rand((B, L, D), generator=gen) * 2 - 1, torch.rand((B, D), generator=gen) * 2 - 1
    gm, gs = torch.randn((B, D), generator=gen), torch.randn((B, 1), generator=gen)
    weights, got = None, []
    for device in devices:
        with torch.cuda.device(device):
            u, d = user.to(device).requires_grad_(True), doc.to(device).requires_grad_(True)
            _, _, model = attention_by_dnn(u.detach()[:1], d.detach()[:1], [256], dnn_activation=act)
            if weights is None:                              # the first model's glorot kernels, with non-zero biases, for both devices
                weights = {n: w.detach().cpu().numpy().copy() for n, w in model.named_weights().items()}
                for n in weights:
                    if n.endswith('bias'):
                        weights[n] = (torch.randn(weights[n].shape, generator=gen) * 0.2).numpy()
            model.set_weights_by_name({n: w.copy() for n, w in weights.items()})
            mat, ssum = model(u, d)
            ks, bs = TD._weights(model)
            grads = torch.autograd.grad((mat * gm.to(device)).sum() + (ssum * gs.to(device)).sum(), [u, d] + ks + bs)
            got.append([t.detach().cpu() for t in (mat, ssum) + tuple(grads)])
    assert all(torch.equal(a, b) for a, b in zip(*got)), 'cuda:0 and cuda:1 disagree'
    nl = 2
    u64, d64 = user.double().requires_grad_(True), doc.double().requires_grad_(True)
    k64 = [torch.from_numpy(weights['layer%d/kernel' % i]).double().requires_grad_(True) for i in range(nl)]
    b64 = [torch.from_numpy(weights['layer%d/bias' % i]).double().requires_grad_(True) for i in range(nl)]
    rmat, rsum = DO.attention_by_dnn(u64, d64, k64, b64, act)
    ref = torch.autograd.grad((rmat * gm.double()).sum() + (rsum * gs.double()).sum(), [u64, d64] + k64 + b64)
    for res in got:
        TD.close(res[0], rmat)
        TD.close(res[1], rsum)
        for a, r in zip(res[2:4 + nl], ref[:2 + nl]):
            TD.close(a, r)
        for a, rb, rk in zip(res[4 + nl:], ref[2 + nl:], ref[2:2 + nl]):
            TD.close(a, rb, scale=max(float(rb.abs().max()), float(rk.abs().max())))


def test_afm_backward_on_a_second_device(devices):
    case = TA._case(6464, 8, 64, 64, 4)
    got = []
    for device in devices:
        with torch.cuda.device(device):
            res = TA._run(TA._layer(case, device), torch.tensor(case['X']).to(device), torch.tensor(case['g']).to(device))
            TA._hold_all(res, case, 'F 64 D 64 A 4 on %s' % device)
            got.append((res[0].cpu(), res[1].cpu(), [w.cpu() for w in res[2]]))
    assert TA._same(*got), 'cuda:0 and cuda:1 disagree'

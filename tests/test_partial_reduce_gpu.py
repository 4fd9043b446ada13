"""GPU: the fp64 tree that turns the per-slab weight-gradient partials of AFMLayer, InteractingLayer and BilinearInteractionLayer into the weight
gradients (csrc/partials.hip), pinned bit for bit.

Each case calls a backward entry point of the C ABI with a workspace the test owns, reads the partial slabs back out of that workspace (the layout
is the one the header of csrc/afm.hip, csrc/autoint.hip and csrc/bilinear.hip documents) and rebuilds every weight gradient on the host in numpy
fp64 in the kernel's order: 64 accumulators, term t goes to accumulator t % 64 in term order, then the 64 accumulators are added in index order,
then one rounding to fp32.  The library's result must be torch.equal to that.  Slab counts below 64 and strictly between 64 and 128 are used, so
that the per-lane loop takes one term and wraps to a second; for bilinear 'all' the term list is slot-major over (slot, row chunk).
The slab count is derived from the documented formula and the workspace query must agree with it, which pins the slab-count rule as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _align(n, a=256):
    return (n + a - 1) // a * a


def _tree(terms):
    """terms: (nterm, n) float32, row t = term t of every element -> (n,) float32."""
    acc = np.zeros((64, terms.shape[1]), np.float64)
    for t in range(terms.shape[0]):
        acc[t % 64] += terms[t].astype(np.float64)
    tot = np.zeros(terms.shape[1], np.float64)
    for c in range(64):
        tot += acc[c]
    return tot.astype(np.float32)


def _floats(ws, byte_off, count):
    return ws[byte_off:byte_off + 4 * count].view(torch.float32).cpu().numpy()


def _dev_f32(rng, dev, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dev)


def _rows_table(_lib, x):
    B, F, D = x.shape
    return _lib.const_array([x.data_ptr() + 4 * f * D for f in range(F)], torch.int64, x.device)


def _hold(got, want, nterm, what):
    assert np.abs(want).max() > 0.0, '%s: the rebuilt gradient is all zeros' % what
    assert torch.equal(got.cpu().reshape(-1), torch.from_numpy(want)), '%s (%d terms per element): the weight gradient is not the documented tree' % (what, nterm)


@pytest.mark.parametrize('B,G', [(20, 5), (300, 75)])
def test_afm(dev, B, G):
    """A slab is [dW (D A) | db (A) | dh (A) | dp (D)] padded to a multiple of 4 floats; one slab per wave of AFM_DW_ROWS = 4 samples."""
    from rec_now_amd import _lib
    F, D, A = 5, 6, 3
    assert G == -(-B // 4)
    rng = np.random.default_rng(B)
    x, dx = _dev_f32(rng, dev, B, F, D), torch.empty((B, F, D), dtype=torch.float32, device=dev)
    W, b, h, p = _dev_f32(rng, dev, D, A, scale=0.4), _dev_f32(rng, dev, A, scale=0.1), _dev_f32(rng, dev, A), _dev_f32(rng, dev, D)
    dout = _dev_f32(rng, dev, B, 1)
    dW, db, dh, dp = (torch.empty_like(t) for t in (W, b, h, p))
    n = D * A + 2 * A + D
    nS = (n + 3) // 4 * 4
    ws_bytes = int(_lib.load().recnow_afm_workspace_bytes(B, F, D, A))
    assert ws_bytes == _align(G * nS * 4)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call('recnow_afm_bwd', _lib.ptr(_rows_table(_lib, x)), F * D, _lib.ptr(_rows_table(_lib, dx)), F * D, F, B, D, A, _lib.ptr(W), _lib.ptr(b),
              _lib.ptr(h), _lib.ptr(p), _lib.ptr(dout), _lib.ptr(dW), _lib.ptr(db), _lib.ptr(dh), _lib.ptr(dp), _lib.ptr(ws), ws_bytes, _lib.stream())
    torch.cuda.synchronize(dev)
    part = _floats(ws, 0, G * nS).reshape(G, nS)[:, :n]
    _hold(torch.cat([t.reshape(-1) for t in (dW, db, dh, dp)]), _tree(part), G, 'AFM B = %d' % B)


@pytest.mark.parametrize('B,G', [(40, 5), (600, 75)])
def test_autoint(dev, B, G):
    """A slab is [dWq | dWk | dWv | dWr], D E floats each; one slab per workgroup of AI_DW_ROWS = 8 samples."""
    from rec_now_amd import _lib
    F, D, H, d = 5, 6, 2, 3
    E = H * d
    assert G == -(-B // 8)
    rng = np.random.default_rng(B)
    x, dx = _dev_f32(rng, dev, B, F, D), torch.empty((B, F, D), dtype=torch.float32, device=dev)
    Ws = [_dev_f32(rng, dev, D, E, scale=0.4) for _ in range(4)]
    dout = _dev_f32(rng, dev, B, F, E)
    dWs = [torch.empty_like(w) for w in Ws]
    n = 4 * D * E
    ws_bytes = int(_lib.load().recnow_autoint_workspace_bytes(B, F, D, H, d, 1))
    assert ws_bytes == _align(G * n * 4)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call('recnow_autoint_bwd', _lib.ptr(_rows_table(_lib, x)), F * D, _lib.ptr(_rows_table(_lib, dx)), F * D, F, B, D, H, d, _lib.ptr(Ws[0]),
              _lib.ptr(Ws[1]), _lib.ptr(Ws[2]), _lib.ptr(Ws[3]), 0, 1, _lib.ptr(dout), _lib.ptr(dWs[0]), _lib.ptr(dWs[1]), _lib.ptr(dWs[2]),
              _lib.ptr(dWs[3]), _lib.ptr(ws), ws_bytes, _lib.stream())
    torch.cuda.synchronize(dev)
    _hold(torch.cat([t.reshape(-1) for t in dWs]), _tree(_floats(ws, 0, G * n).reshape(G, n)), G, 'AutoInt B = %d' % B)


@pytest.mark.parametrize('B,G', [(512, 2), (17920, 70)])
@pytest.mark.parametrize('kind', ['all', 'each', 'interaction'])
def test_bilinear(dev, kind, B, G):
    """The partials follow the [dU] carve ('all', 'each': B (F-1) D floats rounded up to 256 bytes): part[(chunk S + slot) D D + k D + d] with
    S = F - 1 slots ('all', 'each') or P ('interaction') and one row chunk per BIL_DW_ROWS = 256 samples.  'each' and 'interaction' add the G
    chunks of every (slot, k, d); 'all' adds the S G terms (slot t / G, chunk t % G) of every (k, d)."""
    from rec_now_amd import _lib
    F, D = 3, 5
    code = {'all': 0, 'each': 1, 'interaction': 2}[kind]
    S = F * (F - 1) // 2 if kind == 'interaction' else F - 1
    nW = 1 if kind == 'all' else S
    assert G == -(-B // 256)
    rng = np.random.default_rng(B + code)
    xs = [_dev_f32(rng, dev, B, D) for _ in range(F)]
    dx = torch.empty((F, B, D), dtype=torch.float32, device=dev)
    W = _dev_f32(rng, dev, nW, D, D, scale=0.4)
    dout = _dev_f32(rng, dev, B, F * (F - 1) // 2 * D)
    dW = torch.empty_like(W)
    du_bytes = 0 if kind == 'interaction' else _align(B * (F - 1) * D * 4)
    ws_bytes = int(_lib.load().recnow_bilinear_workspace_bytes(B, F, D, code))
    assert ws_bytes == du_bytes + _align(G * S * D * D * 4)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call('recnow_bilinear_bwd', _lib.ptr(_lib.ptr_array(xs, dev)), _lib.ptr(_lib.block_ptr_array(dx, F)), F, B, D, code, _lib.ptr(W),
              _lib.ptr(dout), _lib.ptr(dW), _lib.ptr(ws), ws_bytes, _lib.stream())
    torch.cuda.synchronize(dev)
    part = _floats(ws, du_bytes, G * S * D * D).reshape(G, S, D * D)
    if kind == 'all':
        terms = np.stack([part[t % G, t // G] for t in range(S * G)])               # slot-major
    else:
        terms = part.reshape(G, S * D * D)
    assert (terms.shape[0] > 64) == (G > 64)
    _hold(dW, _tree(terms), terms.shape[0], "bilinear '%s' B = %d" % (kind, B))

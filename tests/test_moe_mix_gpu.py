"""The softmax-gate mixing kernels through the C ABI (recnow_moe_mix_fwd / _bwd), on the cases of tests/_moe_mix_cases.py, inside guard bands (a
sentinel tail past gates, out, dlogits and every dexperts allocation; outputs NaN before the call; each expert an allocation of its own, reached
through the device pointer array), against fp64 on the fp32 inputs:
  gates     each within 1e-5 x the row's largest gate; the gates of every row sum to 1 within 4 ulp
  out       each entry within 1e-5 x sum_n g_n |E_n| of that entry
  dexperts  (with accumulate_dexperts = 1: prefill + contribution) and dlogits: each entry within 1e-5 x its sum of |terms|, and each row
            within 1e-5 x the row's max |ref| (a row whose reference is exactly zero must be exactly zero)
  two runs are bit-identical; N = 65 returns RECNOW_EUNSUPPORTED and writes nothing.
The gates the backward reads are the forward's own fp32 gates: they are an INPUT of recnow_moe_mix_bwd, and its reference is fp64 on them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _moe_mix_cases as C                      # noqa: E402
from _guard import Buf                          # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-5
EUNSUPPORTED = -3


def _ptr_array(dev, bufs):
    import torch
    return torch.tensor([b.ptr for b in bufs], dtype=torch.int64, device=dev)


def run(dev, c, inp):
    """forward, then backward on the forward's gates.  Returns {name: array}; checks every sentinel."""
    import torch
    from rec_now_amd import _lib
    T, B, N, U, form = c['T'], c['B'], c['N'], c['U'], c['form']
    logits, dout = Buf(dev, T * B * N, inp['logits']), Buf(dev, T * B * U, inp['dout'])
    experts = [Buf(dev, B * U, inp['experts'][n]) for n in range(N)]
    ep = _ptr_array(dev, experts)
    gates, out = Buf(dev, T * B * N), Buf(dev, T * B * U)
    st = _lib.stream()
    _lib.call('recnow_moe_mix_fwd', logits.ptr, ep.data_ptr(), T, B, N, U, gates.ptr, out.ptr, st)
    torch.cuda.synchronize()
    dlogits = Buf(dev, T * B * N) if form != 'no_dlogits' else None
    dexperts = None
    if form != 'no_dexperts':
        dexperts = [Buf(dev, B * U, inp['prefill'][n] if form == 'accumulate' else None) for n in range(N)]
        dp = _ptr_array(dev, dexperts)
    _lib.call('recnow_moe_mix_bwd', gates.ptr, ep.data_ptr(), dout.ptr, T, B, N, U, dlogits.ptr if dlogits else None,
              dp.data_ptr() if dexperts else None, 1 if form == 'accumulate' else 0, st)
    torch.cuda.synchronize()
    named = [('logits', logits), ('dout', dout), ('gates', gates), ('out', out)] + [('expert %d' % n, b) for n, b in enumerate(experts)]
    named += [('dlogits', dlogits)] if dlogits else []
    named += [('dexperts %d' % n, b) for n, b in enumerate(dexperts)] if dexperts else []
    for name, b in named:
        bad = b.damaged()
        assert bad == 0, '%s: %d sentinel words past %s changed' % (c['name'], bad, name)
    for n, b in enumerate(experts):          # the inputs are read-only
        assert np.array_equal(b.get((B, U)).view(np.int32), inp['experts'][n].view(np.int32)), '%s: expert %d was written' % (c['name'], n)
    res = {'gates': gates.get((T, B, N)), 'out': out.get((T, B, U))}
    if dlogits:
        res['dlogits'] = dlogits.get((T, B, N))
    if dexperts:
        res['dexperts'] = np.stack([b.get((B, U)) for b in dexperts])
    return res


@pytest.mark.parametrize('c', C.CASES, ids=[c['name'] for c in C.CASES])
def test_moe_mix(dev, c):
    inp = C.make(c)
    got = run(dev, c, inp)
    for k, v in got.items():
        assert np.isfinite(v).all(), '%s: non-finite or unwritten %s' % (c['name'], k)
    g64, out64, mout = C.forward64(inp)
    fr = {'gates': float((np.abs(got['gates'] - g64).max(-1) / (REL * g64.max(-1))).max()),
          'out': C.margins(out64, mout, got['out'], REL)[0]}
    gsum = np.abs(got['gates'].astype(np.float64).sum(-1) - 1.0).max()
    assert gsum <= 4 * 2.0 ** -23, '%s: the gates of a row sum to 1 %+.3g' % (c['name'], gsum)
    ref = C.backward64(c, inp, got['gates'])
    for k in ('dexperts', 'dlogits'):
        if k in got:
            fr[k + ' entry'], fr[k + ' row'] = C.margins(ref[k][0], ref[k][1], got[k], REL)
    assert set(got) == {'gates', 'out'} | ({'dlogits'} if c['form'] != 'no_dlogits' else set()) | ({'dexperts'} if c['form'] != 'no_dexperts' else set())
    worst = max(fr, key=fr.get)
    print('%s: worst margin %.3f of the bound (%s)' % (c['name'], fr[worst], worst))
    over = {k: v for k, v in fr.items() if not v <= 1.0}
    assert not over, '%s: beyond the bound (fraction of it): %r' % (c['name'], over)
    again = run(dev, c, inp)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), '%s: two runs differ in %s' % (c['name'], k)


@pytest.mark.parametrize('entry', ['fwd', 'bwd'])
def test_moe_mix_65_experts_is_unsupported_and_writes_nothing(dev, entry):
    import torch
    from rec_now_amd import _lib
    lib = _lib.load()
    c = dict(name='n65', T=2, B=5, N=C.MOE_MAX_N + 1, U=3, kind='normal', form='plain')
    inp = C.make(c)
    T, B, N, U = c['T'], c['B'], c['N'], c['U']
    experts = [Buf(dev, B * U, inp['experts'][n]) for n in range(N)]
    ep = _ptr_array(dev, experts)
    outs = [Buf(dev, T * B * N), Buf(dev, T * B * U)] + [Buf(dev, B * U) for _ in range(N)]
    if entry == 'fwd':
        logits = Buf(dev, T * B * N, inp['logits'])
        rc = lib.recnow_moe_mix_fwd(logits.ptr, ep.data_ptr(), T, B, N, U, outs[0].ptr, outs[1].ptr, _lib.stream())
    else:
        gates, dout = Buf(dev, T * B * N, np.full((T, B, N), 1.0 / N)), Buf(dev, T * B * U, inp['dout'])
        dp = _ptr_array(dev, outs[2:])
        rc = lib.recnow_moe_mix_bwd(gates.ptr, ep.data_ptr(), dout.ptr, T, B, N, U, outs[0].ptr, dp.data_ptr(), 0, _lib.stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED
    assert all(b.untouched() and b.damaged() == 0 for b in outs)

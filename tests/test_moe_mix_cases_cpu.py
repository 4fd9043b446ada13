"""The cases of tests/test_moe_mix_gpu.py on the CPU: they cover what they claim, and the plain fp32 restatement of the mixing formulas
(tests/_moe_mix_cases.py forward32 / backward32) meets every bound of the GPU test with half of it to spare on the same data -- the bounds are
ones fp32 arithmetic can meet, so a kernel that misses them is wrong."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _moe_mix_cases as C                      # noqa: E402

REL = 1e-5


def test_cases_cover_every_value_forward_and_backward():
    assert len({c['name'] for c in C.CASES}) == len(C.CASES)
    small = [c for c in C.CASES if c['B'] <= 700]
    assert {c['N'] for c in small} == {1, 2, 5, 63, 64} and {c['U'] for c in small} == {1, 63, 64, 65, 130}
    assert {c['T'] for c in small} == {1, 3} and {c['B'] for c in small} == {1, 5, 700}
    assert {c['kind'] for c in C.CASES} == set(C.KINDS) and {c['form'] for c in C.CASES} == set(C.FORMS)
    have = [c for c in small if c['form'] != 'no_dexperts']     # dexperts is produced: every N, U, T, B
    assert {c['N'] for c in have} == {1, 2, 5, 63, 64} and {c['U'] for c in have} == {1, 63, 64, 65, 130}
    assert {c['T'] for c in have} == {1, 3} and {c['B'] for c in have} == {1, 5, 700}
    have = [c for c in small if c['form'] != 'no_dlogits']      # dlogits is produced
    assert {c['N'] for c in have} == {1, 2, 5, 63, 64} and {c['U'] for c in have} == {1, 63, 64, 65, 130}
    assert {c['T'] for c in have} == {1, 3} and {c['B'] for c in have} == {1, 5, 700}
    assert [c for c in C.CASES if c['T'] * c['B'] > C.GRID_ROWS > c['B'] and c['T'] * c['B'] - C.GRID_ROWS < 8]
    assert [c for c in C.CASES if c['B'] > C.GRID_ROWS and c['B'] - C.GRID_ROWS < 8 and c['form'] == 'accumulate']
    assert all(c['T'] == 1 for c in C.CASES if c['U'] == 1)
    assert all(c['N'] <= C.MOE_MAX_N for c in C.CASES)


def test_logit_kinds_are_what_they_say():
    for c in C.CASES:
        lg = C.make(c)['logits'].astype(np.float64)
        if c['kind'] == 'equal':
            assert (lg == lg[..., :1]).all()
        elif c['kind'] == 'spread80':
            assert (np.abs(lg).min(-1) == 80.0).all() and (c['N'] < 2 or ((lg.max(-1) == 80.0) & ((lg == -80.0).sum(-1) == 1)).all())
        elif c['kind'] == 'dominant':
            assert (lg.max(-1) == 1e4).all() and ((lg == 1e4).sum(-1) == 1).all()
        elif c['kind'] == 'offset1e4':
            assert (np.abs(lg).min(-1) > 9.9e3).all() and (lg[..., 0].size < 2 or {-1.0, 1.0} == set(np.sign(lg[..., 0]).reshape(-1)))


@pytest.mark.parametrize('c', C.CASES, ids=[c['name'] for c in C.CASES])
def test_fp32_restatement_meets_half_of_every_bound(c):
    inp = C.make(c)
    g64, out64, mout = C.forward64(inp)
    g32, out32 = C.forward32(inp)
    assert np.isfinite(g32).all() and np.isfinite(out32).all()
    fr = {'gates': float((np.abs(g32 - g64).max(-1) / (REL * g64.max(-1))).max()), 'out': C.margins(out64, mout, out32, REL)[0]}
    assert np.abs(g32.astype(np.float64).sum(-1) - 1.0).max() <= 4 * 2.0 ** -23
    ref = C.backward64(c, inp, g32)
    got = C.backward32(c, inp, g32)
    for k in ('dexperts', 'dlogits'):
        fr[k + ' entry'], fr[k + ' row'] = C.margins(ref[k][0], ref[k][1], got[k], REL)
    over = {k: v for k, v in fr.items() if not v <= 0.5}
    assert not over, '%s: the fp32 restatement uses more than half of the bound: %r' % (c['name'], over)

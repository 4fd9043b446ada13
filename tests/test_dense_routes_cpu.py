"""The MultiDense route table (tests/_dense_routes.py) on the CPU: its declared routes are what the restated predicates of csrc/layers.hip give, every
kernel instance and every boundary of the dispatch has a row, and the integer data of tests/test_dense_routes_gpu.py is exact in fp32 (which is
what makes "bit for bit" a fair demand on the kernels)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _dense_routes as T                      # noqa: E402

ROWS = T.ROUTES
BY_NAME = {r['name']: r for r in ROWS}


def _rows(**kw):
    return [r for r in ROWS if all((v(r[k]) if callable(v) else r[k] == v) for k, v in kw.items())]


def test_names_are_unique_and_rows_say_why():
    assert len(BY_NAME) == len(ROWS)
    for r in ROWS:
        assert len(r['why']) > 20, r['name']
        assert set(r['want']) <= set(T.ALL)
        for k in ('y', 'dkernel', 'dbias', 'dx'):
            assert r[k] in T.KERNEL_INSTANCES[k], (r['name'], k, r[k])


@pytest.mark.parametrize('r', ROWS, ids=[r['name'] for r in ROWS])
def test_declared_routes_are_what_the_predicates_give(r):
    p = T.predicted(r)
    assert {k: r[k] for k in p} == p


def test_every_kernel_instance_has_a_row():
    for k, names in T.KERNEL_INSTANCES.items():
        have = {r[k] for r in ROWS}
        assert set(names) <= have, '%s: no row for %r' % (k, sorted(set(names) - have))
    # the narrow kernel as forward and as dx, with a GEMM on the other side of the same call (the predicates are independent)
    assert _rows(y='narrow', dx='narrow', dkernel='gemm') and _rows(y='narrow', dkernel=lambda v: v.startswith('xty'))
    assert _rows(y='gemm', dx=lambda v: v.startswith('gemm'), dkernel=lambda v: v.startswith('xty'))
    # the register-tile kernel with and without the fused bias sums; the column sum where it is not asked
    assert _rows(dkernel=lambda v: v.startswith('xty'), dbias='xty_fused') and _rows(dkernel=lambda v: v.startswith('xty'), dbias='none')
    assert [r for r in _rows(dkernel='none', dbias='colsum') if T.xty_ok(r['B'], r['D'], r['U'], r['N'])]
    assert [r for r in _rows(dx='none') if T.xty_ok(r['B'], r['D'], r['U'], r['N'])]
    # broadcast and batched dx at N > 1
    assert _rows(dx='gemm_bcast', N=lambda n: n > 1) and _rows(dx='gemm_batched', N=lambda n: n > 1)


def test_every_boundary_has_a_row():
    head = _rows(y=lambda v: v.startswith('head_fwd'))
    assert {64, 256, 260, 1024, 1028, 4096} <= {r['D'] for r in head}
    for d in (60, 66, 4100):
        assert [r for r in _rows(D=d, U=1, N=1) if r['y'] == 'gemm' and r['dkernel'] == 'gemm' and r['dx'] == 'gemm_bcast'], d
    assert {5, 9, 131, 139} <= {r['B'] for r in head}
    assert 131 % T.HEAD_ROWS < 8 and 139 % T.HEAD_ROWS >= 8 and 139 % 8
    # k_head_fwd beyond one trip of its capped grid, the tail without a second row
    big = [r for r in head if r['B'] > T.HEAD_FWD_CAP_ROWS]
    assert big and all(r['B'] - T.HEAD_FWD_CAP_ROWS <= T.HEAD_FWD_CAP_ROWS // 2 for r in big)
    assert [r for r in head if r['dx'] == 'head_dx' and r['B'] * (r['D'] // 4) > T.HEAD_DX_CAP_QUADS]
    assert [r for r in ROWS if r['x_off'] % 4 and r['y'] == 'gemm' and T.head_ok(r['D'], r['U'], r['N'])]
    assert [r for r in ROWS if r['dx_off'] % 4 and r['y'].startswith('head_fwd') and r['dx'] == 'gemm_bcast' and r['dkernel'] == 'gemm']
    assert all(r['x_off'] in (0, 1) and r['dx_off'] in (0, 1) for r in ROWS)
    # narrow
    assert [r for r in _rows(B=T.NARROW_MIN_B - 1) if T.narrow_ok(r['B'] + 1, r['D'], r['U'], r['N']) and r['y'] == 'gemm']
    narrow = _rows(y='narrow')
    assert all(r['B'] % T.ND_ROWS for r in narrow), 'every narrow row has a ragged last tile'
    assert {(4, 4), (64, 32), (32, 64), (128, 32), (32, 128), (12, 20), (24, 32)} <= {(r['D'], r['U']) for r in narrow}
    assert BY_NAME['narrow_12x20']['dkernel'] == 'gemm' and BY_NAME['narrow_24x32']['dkernel'] == 'gemm'
    assert [r for r in _rows(D=132, U=4) if r['y'] == 'gemm' and r['B'] >= T.NARROW_MIN_B]
    assert [r for r in narrow if r['B'] > T.NARROW_CAP_ROWS and (r['D'], r['U']) == (4, 4)]
    # register tiles
    assert {(2, 128), (128, 2)} <= {(r['D'], r['U']) for r in _rows(dkernel='xty<1>', y='gemm')}
    assert [r for r in ROWS if r['dkernel'].startswith('xty') and r['B'] > T.XTY_CAP_ROWS]
    # general route
    assert [r for r in _rows(N=3, U=63) if r['dbias'] == 'colsum'] and [r for r in _rows(N=3, U=64) if r['dbias'] == 'colsum_batched']
    assert [r for r in _rows(U=1, N=2) if r['y'] == 'gemm']
    assert _rows(B=1) and _rows(B=0)


@pytest.mark.parametrize('r', ROWS, ids=[r['name'] for r in ROWS])
def test_integer_data_is_exact_in_fp32(r):
    """Every input is an fp32 number, and for LINEAR and RELU every output entry is a multiple of its grid whose SUM OF |TERMS| stays below 2^24
    grid steps: every partial sum, in whatever order a kernel adds, is then an integer of magnitude below 2^24 on that grid -- exact in fp32."""
    inp = T.integer_inputs(r)
    for a in inp.values():
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    for act in (T.LINEAR, T.RELU):
        out, mag = T.reference(r, inp, act)
        for k in out:
            steps, top = out[k] / T.GRID[k], mag[k] / T.GRID[k]
            assert np.array_equal(steps, np.rint(steps)), (r['name'], k)
            assert top.size == 0 or top.max() < 2 ** 24, (r['name'], k, top.max())
            assert np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k])
        if r['B'] >= 5 and act == T.RELU:
            assert (out['y'] == 0).any() and (out['y'] > 0).any(), 'RELU data has both sides of the kink'

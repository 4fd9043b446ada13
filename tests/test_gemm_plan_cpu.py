"""CPU: the planned route of every row of the exact-fp32 GEMM route table (tests/_gemm_routes.py), asked of recnow_gemm_route -- a host function of
csrc/gemm.hip over csrc/gemm_dispatch.hpp rn_gemm_plan: no device needed.

Each row's descriptor is built by the function the GPU test launches with (_gemm_routes.fill_desc), on synthetic base addresses with the alignment
of a fresh device allocation (256 bytes); the guard bands, leading dimensions and offsets are the GPU test's.  Asserted per row, in the row's
precision (0) and staging: the planned k_gemm instantiation equals the row's `kernel` field by field, and the tag, reduce variant and xcd_remap
equal the row's `extra`.  The table's "instantiated but unreachable" claim: no exact-mode row plans a BK-16 form of XF 9, 41 or 25."""
import ctypes

import pytest

import _gemm_routes as R
from _gemm_routes import ROUTES


def _desc(spec, extra, act=0):
    from rec_now_amd import _lib
    full, cs = R.census_spec(spec, extra)
    geo = R.geometry(full, extra, R.stored_shapes(cs))
    base, nxt = {}, 0x7F0000000000
    for k, g in geo.items():          # consecutive allocations, each on a 256-byte boundary
        base[k] = nxt
        nxt += (4 * g.words + 255) // 256 * 256
    return R.fill_desc(_lib.GemmDesc(), full, extra, act, geo, base)


@pytest.fixture
def lib():
    from rec_now_amd import _lib
    lib = _lib.load()
    prec, stg = lib.recnow_get_gemm_precision(), lib.recnow_get_gemm_staging()
    lib.recnow_set_gemm_precision(0)
    yield lib
    lib.recnow_set_gemm_precision(prec)
    lib.recnow_set_gemm_staging(stg)


def _route(lib, d):
    from rec_now_amd import _lib
    info = _lib.GemmRouteInfo()
    rc = lib.recnow_gemm_route(ctypes.byref(d), lib.recnow_gemm_workspace_bytes(ctypes.byref(d)), ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize('route', ROUTES, ids=[r[0] for r in ROUTES])
def test_planned_route_is_the_rows(lib, route):
    name, kern, spec, extra, _ = route
    lib.recnow_set_gemm_staging(extra.get('staging', 0))
    rc, info = _route(lib, _desc(spec, extra))
    assert rc == 0, '%s: recnow_gemm_route returns %d' % (name, rc)
    R.check_route(name, kern, extra, info)
    assert not (info.bk == 16 and info.xf in (9, 41, 25)), '%s plans a BK-16 form of XF %d' % (name, info.xf)


def test_route_query_return_codes(lib):
    """recnow_gemm_route returns what recnow_gemm returns before its first launch: argument errors, an empty product, a workspace that is too small"""
    from rec_now_amd import _lib
    name, kern, spec, extra, _ = next(r for r in ROUTES if r[0] == 'split16_reduce_quad')
    info = _lib.GemmRouteInfo()
    assert lib.recnow_gemm_route(None, 0, ctypes.byref(info)) == -1
    d = _desc(spec, extra)
    assert lib.recnow_gemm_route(ctypes.byref(d), 0, None) == -1
    assert lib.recnow_gemm_route(ctypes.byref(d), 0, ctypes.byref(info)) == -2                      # 16 slices need slabs
    need = lib.recnow_gemm_workspace_bytes(ctypes.byref(d))
    assert lib.recnow_gemm_route(ctypes.byref(d), need, ctypes.byref(info)) == 0 and info.splitk == 16 and info.kchunk == 256
    assert (info.grid_x, info.grid_y, info.grid_z) == (2, 1, 16)
    d.M = 0
    assert lib.recnow_gemm_route(ctypes.byref(d), need, ctypes.byref(info)) == 0 and info.family == 0      # nothing to launch
    d.M, d.K = 256, 0
    assert lib.recnow_gemm_route(ctypes.byref(d), need, ctypes.byref(info)) == -3
    d.K, d.A = 4096, None
    assert lib.recnow_gemm_route(ctypes.byref(d), need, ctypes.byref(info)) == -1


def test_side_product_over_two_column_tiles_is_tagged_fp32(lib):
    """Split precision: a side product belongs to ONE column tile, so the split kernels refuse N = 256; the fp32 kernel that runs is the one named,
    tag included (it was charged to the bf16x3 roofline before the route was planned ahead of the tag)."""
    spec = dict(M=128, N=256, K=512, sp_r=2)
    extra = {}
    for prec, why in ((0, 'exact'), (1, 'bf16x3')):
        lib.recnow_set_gemm_precision(prec)
        rc, info = _route(lib, _desc(spec, extra))
        assert rc == 0 and R.planned_kernel(info) == R.kname(128, 128, 32, True, False, False, 0, 0, 9), (why, rc, info.family)
        assert info.tag == R.T128 and info.splitk == 2 and info.grid_y == 2, (why, info.tag, info.splitk)
    # one column tile: a split kernel takes it (k_gemm_s3, or k_gemm_split under RECNOW_SPLIT_LEAN=0)
    rc, info = _route(lib, _desc(dict(spec, N=128), extra))
    assert rc == 0 and info.family in (4, 5) and info.tag == 8, (rc, info.family, info.tag)

"""CPU: the host side of SparseGNNLayer's dense route (rec_now_amd/layers/sparse_gnn_layer.py): the `route` keyword, the rule behind
route='auto', and the C ABI of csrc/sparse_gnn_dense.hip (declared, exported, bound; the workspace query is host-only)."""
import pytest

from rec_now_amd.layers import sparse_gnn_layer as S
from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer


def ring(F):
    return {i: sorted({(i - 1) % F, (i + 1) % F}) for i in range(F)}


def complete(F):
    return {i: [j for j in range(F) if j != i] for i in range(F)}


def test_route_keyword_is_validated():
    for route in ('edges', 'dense', 'auto'):
        assert SparseGNNLayer(list(range(4)), ring(4), route=route).route == route
    for bad in ('Dense', 'mfma', None, 1):
        with pytest.raises(ValueError, match='route'):
            SparseGNNLayer(list(range(4)), ring(4), route=bad)
    with pytest.raises(TypeError):
        SparseGNNLayer(list(range(4)), ring(4), None, 1, True, 'tanh', 'dense')       # keyword only


def test_default_route_is_edges():
    layer = SparseGNNLayer(list(range(32)), complete(32))
    assert layer.route == 'edges' and layer.chosen_route() == 'edges'
    assert SparseGNNLayer(list(range(32)), complete(32), route='dense').chosen_route() == 'dense'


def test_auto_picks_by_field_count_and_edges():
    """The measured table (profiles/gnn_layer_bench.txt): at F 32 the dense route wins from the ring (E 64) on, at F 64 from E 512 on; sparser
    graphs were not measured and stay on the edge route; above 64 fields there is only the dense route."""
    chain = {i: [i - 1] for i in range(1, 32)}                                      # in-degree <= 1, E = 31
    assert SparseGNNLayer(list(range(32)), chain, route='auto').chosen_route() == 'edges'
    assert SparseGNNLayer(list(range(32)), {}, route='auto').chosen_route() == 'edges'
    assert SparseGNNLayer(list(range(32)), ring(32), route='auto').chosen_route() == 'dense'
    assert SparseGNNLayer(list(range(32)), complete(32), route='auto').chosen_route() == 'dense'
    assert SparseGNNLayer(list(range(64)), ring(64), route='auto').chosen_route() == 'edges'       # E 128 < 512
    assert SparseGNNLayer(list(range(64)), complete(64), route='auto').chosen_route() == 'dense'
    for nbrs in ({}, {0: [1]}, ring(65), complete(65)):
        assert SparseGNNLayer(list(range(65)), nbrs, route='auto').chosen_route() == 'dense'
    # the rule itself: one function, thresholds in edges per field count, rising field counts
    assert S.auto_route(65, 0) == 'dense' and S.auto_route(128, 5) == 'dense'
    fields = [f for f, _ in S.DENSE_MIN_EDGES]
    assert fields == sorted(fields) and fields[-1] == S.MAX_FIELDS
    for f, edges in S.DENSE_MIN_EDGES:
        assert 1 <= edges <= f * f
        assert S.auto_route(f, edges) == 'dense' and S.auto_route(f, edges - 1) == 'edges'
        assert S.auto_route(f, 0) == 'edges'


def test_dense_edge_upload_is_sources_then_destinations():
    layer = SparseGNNLayer([0, 1, 2], {0: [2], 1: [2, 0]}, route='dense')
    layer.build(None)
    assert layer.indices == [[0, 1], [2, 0], [2, 1]]
    assert layer._edges == (0, 2, 2, 1, 0, 1)
    empty = SparseGNNLayer([0, 1, 2], {}, route='dense')
    empty.build(None)
    assert empty.indices == [] and len(empty._edges) >= 1          # never an empty upload


def test_abi_has_the_dense_entry_points():
    from rec_now_amd import _lib
    lib = _lib.load()
    for name in ('recnow_sparse_gnn_dense_fwd', 'recnow_sparse_gnn_dense_bwd', 'recnow_sparse_gnn_dense_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.recnow_abi_version() >= 15


def test_workspace_query():
    """Host-only: the dense matrices (n_sets, 2, FP, FP), FP = F rounded up to 32, and for the backward the rows of dM: at most 1024 rows and
    32 MB (but 16 rows).  No argument is a batch size."""
    from rec_now_amd import _lib
    q = _lib.load().recnow_sparse_gnn_dense_workspace_bytes
    mats = lambda F, n: n * 2 * (-(-F // 32) * 32) ** 2 * 4
    for F, E, n in ((1, 1, 1), (32, 992, 3), (33, 40, 1), (64, 4096, 8), (65, 7, 3), (128, 128 * 127, 8)):
        fwd, bwd = q(F, E, n, 0), q(F, E, n, 1)
        assert mats(F, n) <= fwd < mats(F, n) + 4096
        row = mats(F, n) // 2
        rows = max(16, min(1024, (32 << 20) // row))
        assert fwd + rows * row <= bwd < fwd + rows * row + 4096
    assert q(32, 0, 1, 1) == q(32, 0, 1, 0)                        # no edges: no weight gradient, no rows
    assert q(129, 5, 1, 0) == 0 and q(0, 0, 1, 0) == 0

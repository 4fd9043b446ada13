"""Inputs and invariants of `build_segments`, shared by tests/test_pairwise_gpu.py, tests/test_grouping_routes_gpu.py and tools/group_bits.py."""
import numpy as np

# (B, kind) of test_build_segments_invariants_mid_sizes
MID_CASES = [(30000, 'f32'), (30000, 'pair_f32'), (70000, 'i64'), (9000, 'f64'), (300000, 'f32_wide'), (524288, 'pair_mixed'), (12345, 'all_equal'),
             # float ids that are all small non-negative integers are sorted by their integer images (fewer digit passes), on one workgroup and on
             # 2048- / 4096-key tiles; ids that break the rule (>= 2^24, negative, fractional) as before
             (70000, 'int_img'), (262144, 'int_img_big'), (40000, 'int_over'), (40000, 'int_neg'), (40000, 'frac'), (20000, 'signed_zero_ints'),
             (8000, 'int_img'), (8000, 'frac'), (8192, 'int_img_big')]

# the sizes at which the grouping changes route: one workgroup | cooperative, 2048 | 4096 keys per workgroup, cooperative | multi-launch chain
BOUNDARY_SIZES = [8192, 8193, 262143, 262144, 1048576, 1048577]


def mid_size_groups(B, kind):
    """The group id arrays of one case of test_build_segments_invariants_mid_sizes."""
    rng = np.random.default_rng(B % 1000 + len(kind))
    if kind == 'f32':
        gs = [rng.integers(0, 500, B).astype(np.float32)]
        gs[0][::1013] = np.nan
        gs[0][5::2027] = np.inf
    elif kind == 'pair_f32':
        gs = [rng.integers(0, 40, B).astype(np.float32), rng.integers(0, 7, B).astype(np.float32)]
    elif kind == 'i64':
        gs = [rng.integers(-2 ** 40, 2 ** 40, 300)[rng.integers(0, 300, B)].astype(np.int64)]
    elif kind == 'f64':
        gs = [rng.normal(size=200)[rng.integers(0, 200, B)].astype(np.float64)]
    elif kind == 'f32_wide':
        gs = [rng.normal(size=5000).astype(np.float32)[rng.integers(0, 5000, B)]]
    elif kind == 'pair_mixed':
        gs = [rng.integers(0, 3000, B).astype(np.int32), rng.integers(0, 3, B).astype(np.float32)]
    elif kind == 'int_img':
        gs = [rng.integers(0, 4096, B).astype(np.float32)]
    elif kind == 'int_img_big':
        gs = [rng.integers(0, 2 ** 24, 3000)[rng.integers(0, 3000, B)].astype(np.float32)]
        gs[0][:4] = [0.0, 16777215.0, 1.0, 16777215.0]
    elif kind == 'int_over':
        gs = [rng.integers(0, 300, B).astype(np.float32)]
        gs[0][::97] = 16777216.0 + 2.0 * rng.integers(0, 5, len(gs[0][::97]))
    elif kind == 'int_neg':
        gs = [rng.integers(-50, 50, B).astype(np.float32)]
    elif kind == 'frac':
        gs = [rng.integers(0, 300, B).astype(np.float32) + 0.5]
    elif kind == 'signed_zero_ints':
        gs = [rng.integers(0, 10, B).astype(np.float32)]
        gs[0][gs[0] == 0][::2] = -0.0
        gs[0][::31] = -0.0
    else:
        gs = [np.full(B, -0.0, np.float32)]
        gs[0][::2] = 0.0                                            # -0.0 and +0.0 are one group
    return gs


def boundary_groups(B, dtype):
    """One id tensor for a route boundary size: int32 ids, or float32 ids holding a NaN and an inf."""
    rng = np.random.default_rng(B % 1000 + 17)
    g = rng.integers(0, 3000, B).astype(dtype)
    if dtype == np.float32:
        g[B // 3] = np.nan
        g[B // 2] = np.inf
    return [g]


def segment_arrays(seg, B):
    """(order, seg_id, seg_first[:n_seg + 1], super_id, n_seg[2]) of a Segments as host arrays."""
    order, seg_id, super_id = (t.cpu().numpy()[:B] for t in (seg.order, seg.seg_id, seg.super_id))
    n_seg = seg.n_seg.cpu().numpy()
    return order, seg_id, seg.seg_first.cpu().numpy()[:int(n_seg[0]) + 1], super_id, n_seg


def check_segments(seg, gs, B):
    """The order is a permutation, rows of a segment are ascending (stable sort), rows share a segment iff every key word matches (NaN / inf
    ids are segments of their own), seg_first / n_seg are consistent, and the super segments follow the FIRST group tensor only."""
    order, seg_id, super_id = (t.cpu().numpy()[:B] for t in (seg.order, seg.seg_id, seg.super_id))
    n_seg, n_super = (int(v) for v in seg.n_seg.cpu().numpy())
    seg_first = seg.seg_first.cpu().numpy()[:n_seg + 1]
    assert n_seg >= 1 and np.array_equal(np.sort(order), np.arange(B))
    assert seg_first[0] == 0 and seg_first[-1] == B and np.all(np.diff(seg_first) > 0)
    assert np.array_equal(seg_id, np.repeat(np.arange(n_seg), np.diff(seg_first)))
    same_seg = seg_id[1:] == seg_id[:-1]
    assert np.all(order[1:][same_seg] > order[:-1][same_seg])                       # stable: ascending rows inside a segment

    def canon(g):
        g = g[order]
        solo = ~np.isfinite(g) if g.dtype.kind == 'f' else np.zeros(B, bool)
        return np.where(g == 0, 0, g) if g.dtype.kind == 'f' else g, solo

    keys = [canon(g) for g in gs]
    solo = np.zeros(B, bool)
    for _, so in keys:
        solo |= so
    eq_all = np.ones(B - 1, bool)
    for k, _ in keys:
        eq_all &= k[1:] == k[:-1]
    eq_all &= ~(solo[1:] | solo[:-1])
    assert np.array_equal(same_seg, eq_all)                                           # neighbours share a segment iff all words match
    # globally: the number of segments = distinct composite keys among the finite rows + one per solo row
    fin = ~solo
    comp = np.stack([k[fin].astype(np.float64) if k.dtype.kind == 'f' else k[fin] for k, _ in keys], 1)
    assert n_seg == len(np.unique(comp, axis=0)) + int(solo.sum())
    eq_first = (keys[0][0][1:] == keys[0][0][:-1]) & ~(solo[1:] | solo[:-1])
    assert np.array_equal(super_id[1:] == super_id[:-1], eq_first) and n_super == super_id[-1] + 1

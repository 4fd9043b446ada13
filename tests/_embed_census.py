"""Route census of the pooled-embedding kernels (rec_now_amd/csrc/embed.hip): pure numpy, no torch, no GPU.

A restatement of the ROUTING of those kernels, not of their arithmetic (that is tests/_embed_oracle.py):
  backward  recnow_embed_rows_bwd / _direct walk the id-sorted entries in chunks of EMB_CH; which of the three writers (chunk walk, lane-group
            join, workgroup join) produces a segment's row, and from which piece slots, follows from where the segment's run of sorted entries
            falls relative to the chunk grid.  classify_segments names those alignments, layouts(D) is the case table whose segments reach every
            one of them by construction, build_layout turns a list of segment lengths into the arrays the kernel takes;
  forward   recnow_embed_pool_fwd picks the 16-byte-gather or the scalar kernel and 4 / 2 / 1 waves per workgroup (or refuses);
            fwd_route restates that choice, fwd_cases() is the case table, fwd_inputs its data, fwd_classes what the data reaches.
tests/test_embed_census_cpu.py holds the tables to the class lists; tests/test_embed_kernels_gpu.py runs them.
"""
import numpy as np

EMB_CH = 32          # sorted entries per chunk
EMB_JSHORT = 16      # a segment spanning fewer chunk boundaries than this is joined by one lane group
EMB_JU = 16          # unroll of the workgroup join
KEY_NOT_POOLED = -(1 << 63)

D_CLASSES = (1, 12, 16, 17, 32, 33, 64, 65, 130)


def LPE(D):
    """lanes per entry of the chunk walk = dims lanes of the join"""
    return 16 if D <= 16 else 32 if D <= 32 else 64


def NPL(D):
    """piece lanes of the workgroup join"""
    return 256 // LPE(D)


SEGMENT_CLASSES = (
    'whole', 'whole_at_chunk_start', 'whole_at_chunk_end', 'whole_one_chunk', 'whole_inside',
    'lane_join', 'lane_join_slot0', 'lane_join_slot1', 'lane_join_ends_at_chunk_end', 'lane_join_full_middle', 'lane_join_span_15',
    'wg_join', 'wg_join_slot0', 'wg_join_slot1', 'wg_join_ends_at_chunk_end', 'wg_join_full_middle', 'wg_join_span_16',
    'wg_join_unrolled', 'wg_join_ragged_tail', 'wg_join_even_tail', 'wg_join_lane_tail_15', 'wg_join_lane_no_tail',
)
LAYOUT_CLASSES = ('last_chunk_partial', 'last_chunk_full', 'one_chunk_no_join', 'not_pooled_last', 'all_pooled')


def classify_segments(lengths, D):
    """One set of SEGMENT_CLASSES per segment of the sorted layout whose segments have these lengths, in this order."""
    npl = NPL(D)
    out, f = [], 0
    for n in lengths:
        assert n >= 1
        e = f + n                                             # sorted positions f .. e - 1
        c0, c1 = f // EMB_CH, (e - 1) // EMB_CH
        at_start, at_end = f % EMB_CH == 0, e % EMB_CH == 0
        cls = set()
        if c0 == c1:
            cls.add('whole')
            if at_start:
                cls.add('whole_at_chunk_start')
            if at_end:
                cls.add('whole_at_chunk_end')
            if at_start and at_end:
                cls.add('whole_one_chunk')
            if not at_start and not at_end:
                cls.add('whole_inside')
        else:
            span = c1 - c0
            k = 'wg_join' if span >= EMB_JSHORT else 'lane_join'
            cls.add(k)
            cls.add(k + ('_slot0' if at_start else '_slot1'))
            if at_end:
                cls.add(k + '_ends_at_chunk_end')
            if span >= 2:
                cls.add(k + '_full_middle')
            if span == EMB_JSHORT - 1:
                cls.add('lane_join_span_15')
            if span == EMB_JSHORT:
                cls.add('wg_join_span_16')
            if k == 'wg_join':
                if span >= (EMB_JU + 1) * npl:
                    cls.add('wg_join_unrolled')
                cls.add('wg_join_ragged_tail' if (span + 1) % npl else 'wg_join_even_tail')
                left = join_lane_pieces(span, npl)
                if any(v % EMB_JU == EMB_JU - 1 for v in left):
                    cls.add('wg_join_lane_tail_15')
                if any(v >= EMB_JU and v % EMB_JU == 0 for v in left):
                    cls.add('wg_join_lane_no_tail')
        out.append(frozenset(cls))
        f = e
    return out


def join_lane_pieces(span, npl):
    """Pieces each of the npl piece lanes of the workgroup join adds in its unrolled loop and its tail: lane p owns the chunks c0 + p, c0 + p + npl,
    ... up to c1 = c0 + span, and lane 0 takes the first one (the only piece that may sit in slot 1) on its own before the loop.  The loop takes
    EMB_JU pieces per turn while that many are left, the tail the rest: a lane with EMB_JU - 1 left is the longest tail (one piece short of a
    turn), a lane with a whole multiple left has no tail."""
    return [(span - p) // npl + 1 - (1 if p == 0 else 0) for p in range(npl) if p <= span]


def not_pooled_last(lengths):
    """The case tables give a layout of more than one segment a last segment of entries that are not pooled (key KEY_NOT_POOLED, target -1)."""
    return len(lengths) > 1


def classify_layout(lengths):
    N = sum(lengths)
    cls = {'last_chunk_partial' if N % EMB_CH else 'last_chunk_full'}
    if N <= EMB_CH:
        cls.add('one_chunk_no_join')
    cls.add('not_pooled_last' if not_pooled_last(lengths) else 'all_pooled')
    return frozenset(cls)


def main_layout(D):
    """28 segments.  Each comment gives the sorted positions the segments of its line end at, the chunks they lie in and what they are there for;
    MAIN_ROLES pins the outcome."""
    npl, C = NPL(D), EMB_CH
    return [5, 27,                    # -> 32    chunk 0: whole from the chunk start; whole up to the chunk end
            32,                       # -> 64    chunk 1: exactly one chunk
            1, 31,                    # -> 96    chunk 2: a single entry at the chunk start; whole up to the chunk end
            33,                       # -> 129   chunks 3 .. 4: lane join, first piece in slot 0, one boundary
            31,                       # -> 160   chunk 4: whole up to the chunk end, after a cut run in the same chunk
            40, 24,                   # -> 224   chunks 5 .. 6: lane join from slot 0; whole up to the chunk end
            64,                       # -> 288   chunks 7 .. 8: lane join of two full chunks: slot 0, ends at a chunk end
            3, 70,                    # -> 361   chunks 9 .. 11: lane join from slot 1 with a full middle chunk
            15 * C - 7,               # -> 834   chunks 11 .. 26: 15 boundaries, the longest lane join (slot 1)
            16 * C - 20,              # -> 1326  chunks 26 .. 41: 15 boundaries again, the next owner boundary
            10,                       # -> 1336  chunk 41: whole, strictly inside
            16 * C + 1,               # -> 1849  chunks 41 .. 57: 16 boundaries, the shortest workgroup join (slot 1)
            17 * C + 9,               # -> 2402  chunks 57 .. 75: workgroup join over 18 boundaries
            32 * 15,                  # -> 2882  chunks 75 .. 90: 480 entries off the grid: 15 boundaries, lane join
            7,                        # -> 2889
            32 * 16,                  # -> 3401  chunks 90 .. 106: 512 entries off the grid: 16 boundaries, workgroup join
            11,                       # -> 3412
            32 * 17,                  # -> 3956  chunks 106 .. 123: 17 boundaries, workgroup join
            2,                        # -> 3958
            (17 * npl + 3) * C + 5,   # chunks 123 ..: every piece lane of the workgroup join runs its unrolled body, then a tail
            1, 1, 29,                 # two single entries and a lane join over the last full boundary
            19]                       # not pooled: 6 entries in the last full chunk, 13 in the partial one: a lane join of zero rows


# what each segment of main_layout is, whatever D: deleting or resizing a segment moves the ones behind it off these roles
MAIN_ROLES = ('whole', 'whole', 'whole', 'whole', 'whole', 'lane_join_slot0', 'whole', 'lane_join_slot0', 'whole', 'lane_join_slot0', 'whole',
              'lane_join_slot1', 'lane_join_slot1', 'lane_join_slot1', 'whole', 'wg_join_slot1', 'wg_join_slot1', 'lane_join_slot1', 'whole',
              'wg_join_slot1', 'whole', 'wg_join_slot1', 'whole', 'wg_join_slot1', 'whole', 'whole', 'lane_join_slot1', 'lane_join_slot1')
MAIN_N = {16: 12813, 32: 8461, 64: 6285}          # by LPE; N % 32 == 13 in each


def role(cls):
    """'whole', or the join and the slot of its first piece"""
    return 'whole' if 'whole' in cls else [c for c in cls if c.endswith(('_slot0', '_slot1'))][0]


def aligned_layout(D):
    """Segments that START on a chunk start and span 15 / 16 / 17 boundaries (slot 0 in both joins), end exactly at chunk ends, a workgroup join
    whose piece count is a multiple of NPL, and N a multiple of the chunk."""
    npl, C = NPL(D), EMB_CH
    k = (EMB_JU + 2) * npl                                    # pieces: a multiple of NPL past the unrolled threshold
    return [15 * C + 1,               # chunks 0 .. 15 from a chunk start: lane join, slot 0, span 15
            C - 1,                    # whole, ends at the chunk end                                                       -> 16 C
            16 * C,                   # 16 whole chunks: lane join slot 0, span 15, ends at a chunk end                    -> 32 C
            16 * C + 1,               # workgroup join, slot 0, span 16
            C - 1,                    #                                                                                    -> 49 C
            17 * C,                   # workgroup join, slot 0, span 16, ends at a chunk end                               -> 66 C
            7, 17 * C + (C - 7),      # workgroup join, slot 1, ends at a chunk end                                        -> 84 C
            k * C,                    # workgroup join, slot 0, unrolled, piece count a multiple of NPL, ends at a chunk end
            3, 2 * C - 3 + 16,        # lane join slot 1
            16]                       # not pooled, whole, ends at the chunk end = N


def unroll_layout(D):
    """The two edges of the workgroup join's unrolled loop: 15 NPL + 1 pieces -- every piece lane is left with EMB_JU - 1 = 15 pieces, one short
    of a turn of the loop, so all of them go through the tail -- and 16 NPL + 1 pieces: exactly one turn for every lane and no tail."""
    npl, C = NPL(D), EMB_CH
    return [9,
            (EMB_JU - 1) * npl * C + 1,       # from position 9: 15 NPL boundaries
            5,
            EMB_JU * npl * C + 1,             # 16 NPL boundaries
            40,                               # a lane join behind it: pieces in the chunks right after the long segment
            7]                                # not pooled


TINY_LAYOUTS = ([1], [32], [33], [7, 25], [40])


LAYOUT_NAMES = ('main', 'aligned', 'unroll') + tuple('tiny' + '_'.join(str(v) for v in t) for t in TINY_LAYOUTS)


def layouts(D):
    """The backward case table for row width D, in the order of LAYOUT_NAMES."""
    return [main_layout(D), aligned_layout(D), unroll_layout(D)] + [list(t) for t in TINY_LAYOUTS]


def build_layout(lengths, C, T, seed=0, pooled_last=None, keys=None):
    """The arrays recnow_embed_rows_bwd takes for a sorted layout with these segment lengths: order (sorted position -> entry; the entries of a
    segment ascending, the segments scattered over [0, N) by a seeded permutation), seg_id, seg_first (N + 1 words), n_seg (2 words), key (per
    ENTRY; ascending per segment, with gaps) and the target index t per entry in [0, T) -- -1 and KEY_NOT_POOLED for the entries of the last
    segment where not_pooled_last(lengths).  `keys` overrides the per-segment keys."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    S, N = len(lengths), int(lengths.sum())
    first = np.concatenate([[0], np.cumsum(lengths)])
    perm = rng.permutation(N)
    order = np.concatenate([np.sort(perm[first[s]:first[s + 1]]) for s in range(S)]).astype(np.int32)
    seg_id = np.repeat(np.arange(S, dtype=np.int32), lengths)
    seg_first = np.full(N + 1, N, np.int32)
    seg_first[:S + 1] = first
    sentinel = not_pooled_last(lengths) if pooled_last is None else not pooled_last
    if keys is None:
        seg_keys = np.cumsum(rng.integers(1, 4, S)).astype(np.int64) - 1      # ascending, gaps of 0 .. 2 unused rows
        if sentinel:
            seg_keys[-1] = KEY_NOT_POOLED
    else:
        seg_keys = np.asarray(keys, np.int64)
        assert seg_keys.shape == (S,)
    key = np.empty(N, np.int64)
    key[order] = seg_keys[seg_id]
    t = rng.integers(0, T, N).astype(np.int32)
    if sentinel:
        t[order[first[S - 1]:]] = -1
    return dict(N=N, S=S, C=C, T=T, B=-(-N // C), order=order, seg_id=seg_id, seg_first=seg_first, n_seg=np.array([S, S], np.int32),
                key=key, seg_keys=seg_keys, t=t, first=first, lengths=lengths)


def bwd_values(lay, D, family, mean, use_w, seed=0):
    """dout (B, T, D), weights (N,) or None, cnt (B, T) or None.  'exact': integers in [-8, 8], weights from {0.5, 1, 2}, counts from
    {1, 2, 4, 8} -- every term is a multiple of 1/16, so while sum |term| < 2^24 / 16 every fp32 sum is exact in any order.
    'float': normal dout, weights uniform(-1.5, 1.5), counts 1 .. 9."""
    rng = np.random.default_rng([seed, D, int(mean), int(use_w), family == 'exact'])
    B, T, N = lay['B'], lay['T'], lay['N']
    if family == 'exact':
        dout = rng.integers(-8, 9, (B, T, D)).astype(np.float32)
        w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), N) if use_w else None
        cnt = rng.choice(np.array([1.0, 2.0, 4.0, 8.0], np.float32), (B, T)) if mean else None
    else:
        dout = rng.standard_normal((B, T, D)).astype(np.float32)
        w = rng.uniform(-1.5, 1.5, N).astype(np.float32) if use_w else None
        cnt = rng.integers(1, 10, (B, T)).astype(np.float32) if mean else None
    return dout, w, cnt


EXACT_UNIT = 1.0 / 16.0           # every term of the exact family is a whole multiple of this
EXACT_LIMIT = float(1 << 24)      # ... and every partial sum stays below this many units


def direct_keys(lengths, D, V, oob):
    """Per-segment keys of the direct route (the key IS the table row): ascending, odd rows only.  With oob the first six segments carry keys
    below 0 and the segments from the last workgroup join on carry keys >= V.  The keys of join segments stay within DIRECT_GUARD_ROWS of the
    table (the test's table has that many guard rows on either side, so a join that ignored the bounds would write into them and not into
    foreign memory); whole segments at the two ends also get keys far outside, whose low 32 bits name a row of the table."""
    S = len(lengths)
    cls = classify_segments(lengths, D)
    keys = np.arange(S, dtype=np.int64) * 2 + 1
    assert keys[-1] < V
    if oob:
        lo = min(DIRECT_GUARD_ROWS, S // 2)
        keys[:lo] = np.arange(-lo, 0)
        wg = [s for s in range(S) if 'wg_join' in cls[s]]
        hi = max(wg[-1] if wg else S - 1, lo)
        assert S - hi <= DIRECT_GUARD_ROWS
        keys[hi:] = V + np.arange(S - hi)
        if lo and 'whole' in cls[0]:
            keys[0] = -(1 << 40) + 3
        if 'whole' in cls[S - 1] and S - 1 > hi:
            keys[S - 1] = (1 << 40) + 1
    return keys


DIRECT_GUARD_ROWS = 6


# ---- forward -------------------------------------------------------------------------------------------------------------------------------

def fwd_route(T, D, aligned=True):
    """(kernel, waves per workgroup) of recnow_embed_pool_fwd, waves None = RECNOW_EUNSUPPORTED"""
    per_wave = (T * D + T) * 4
    w = 4
    while w > 1 and per_wave * w > 65536:
        w >>= 1
    if per_wave * w > 65536:
        return None, None
    v4 = D in (4, 8, 16, 32, 64) and T % 4 == 0 and aligned
    return ('v4' if v4 else 'scalar'), w


def fwd_groups(T, D, aligned=True):
    """lane groups per wave: targets are dealt to them round robin"""
    if fwd_route(T, D, aligned)[0] == 'v4':
        return 64 // (D // 4)
    gs = 1
    while gs < D and gs < 64:
        gs <<= 1
    return 64 // gs


def fwd_cases():
    """(T, D, C, B, V) of the forward case table"""
    return [(24, 16, 130, 40, 50),       # v4, 4 waves
            (96, 64, 65, 5, 30),         # v4, 2 waves
            (200, 64, 64, 3, 30),        # v4, 1 wave
            (8, 4, 65, 11, 20), (4, 8, 63, 13, 20), (12, 32, 130, 5, 40),      # v4 at the other widths
            (23, 16, 63, 7, 50),         # scalar because T % 4 != 0
            (70, 12, 130, 4, 40), (9, 1, 1, 40, 9), (3, 70, 65, 6, 11), (5, 130, 64, 9, 7),
            (100, 70, 63, 3, 12),        # scalar, 2 waves
            (90, 130, 130, 3, 12),       # scalar, 1 wave
            (260, 64, 63, 3, 10)]       # more LDS than a workgroup has: refused


FWD_ROUTES = (('v4', 4), ('v4', 2), ('v4', 1), ('scalar', 4), ('scalar', 2), ('scalar', 1), (None, None))
FWD_C = (1, 63, 64, 65, 130)
FWD_COUNTS = ('0', '1', '4', '5', '>8')
_PATTERN = (0, 1, 4, 5, 9, 2, 13)        # entries of targets 0 .. 6 in row 0 and of targets T-1 .. T-7 in the last row, where C allows


def fwd_inputs(case, family, use_w, seed=0):
    """seg (B, C) target index or -1, rows (B, C) table rows (a few outside [0, V)), weights (B, C) or None, table (V, D)."""
    T, D, C, B, V = case
    rng = np.random.default_rng([seed, T, D, C, B, family == 'exact'])
    seg = rng.integers(-1, T, (B, C)).astype(np.int32)
    for b, tl in ((0, list(range(T))), (B - 1, list(range(T - 1, -1, -1)))):
        fill = []
        for t, n in zip(tl, _PATTERN):
            if len(fill) + n > C:
                break
            fill += [t] * n
        if fill:                                                      # the other columns of such a row are not pooled
            seg[b] = np.array(fill + [-1] * (C - len(fill)), np.int32)[rng.permutation(C)]
    rows = rng.integers(0, V, (B, C)).astype(np.int64)
    rows[rng.random((B, C)) < 0.04] = -1
    rows[rng.random((B, C)) < 0.04] = V
    rows[rng.random((B, C)) < 0.02] = (1 << 33) + 2
    if family == 'exact':
        table = rng.integers(-8, 9, (V, D)).astype(np.float32)
        w = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), (B, C)) if use_w else None
    else:
        table = rng.standard_normal((V, D)).astype(np.float32)
        w = rng.uniform(-1.5, 1.5, (B, C)).astype(np.float32) if use_w else None
    return seg, rows, w, table


def fwd_classes(case):
    """What a forward case reaches: its route, its C, the per-(row, target) entry counts of FWD_COUNTS, and the shape properties."""
    T, D, C, B, V = case
    cls = {('route',) + fwd_route(T, D), ('C', C)}
    if fwd_route(T, D)[0] is None:
        return cls
    if fwd_route(T, D)[0] == 'v4':
        cls.add(('route',) + fwd_route(T, D, aligned=False))          # the same shape from a misaligned table
    seg = fwd_inputs(case, 'exact', True)[0]
    n = np.zeros((B, T), np.int64)
    bb, cc = np.nonzero(seg >= 0)
    np.add.at(n, (bb, seg[bb, cc]), 1)
    for v in np.unique(n):
        if str(v) in FWD_COUNTS:
            cls.add(('count', str(v)))
        if v > 8:
            cls.add(('count', '>8'))
    if T % fwd_groups(T, D):
        cls.add('T_not_multiple_of_groups')
    if T > 64:
        cls.add('T_over_64')
    if C > 64:
        cls.add('several_rounds')
    if D > 64:
        cls.add('D_over_64')
    return cls


FWD_CLASSES = (tuple(('route',) + r for r in FWD_ROUTES) + tuple(('C', c) for c in FWD_C) + tuple(('count', c) for c in FWD_COUNTS)
               + ('T_not_multiple_of_groups', 'T_over_64', 'several_rounds', 'D_over_64'))

BWD_WEIGHTS_D = (1, 4, 5, 8, 9, 16, 33, 64, 65, 130)

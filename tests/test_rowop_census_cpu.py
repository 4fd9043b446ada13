"""CPU: the route table of FM, InnerPNN and attention_by_dot_product (tests/_rowop_routes.py) and its census (tests/_rowop_census.py) are what
tests/test_rowop_routes_gpu.py takes them for.
  * the Python mirrors of the three route choices equal recnow_fm_route / recnow_inner_pnn_route / recnow_attention_dot_route (host functions: no
    device needed) on every row and over a sweep that straddles every threshold;
  * the table reaches every code the sweep can reach, and every loop has a one-pass row and a row with a ragged last pass after the first;
  * the closed forms the scales come from equal oracle/dense_ref under fp64 autograd, and every scale is at least the sum it belongs to;
  * census: on every row every sum any kernel forms keeps sum |terms| < 2^24 on the first ladder entry, and an fp32 restatement in the kernels'
    factorisation returns the fp64 values to the bit; with each planted mistake it does not;
  * random data: the fp32 restatement stays under half the 1e-5 bound on every row (the data, not the bound, was chosen for that);
  * _lib.aligned_fields copies exactly the misaligned fields of a float4 route."""
import numpy as np
import pytest
import torch

import _rowop_census as C
import _rowop_routes as T


def _lib():
    from rec_now_amd import _lib
    return _lib.load()


def test_table_matches_mirror_and_query():
    lib = _lib()
    for r in T.ROUTES:
        for which, want in ((0, r['fwd']), (1, r['bwd'])):
            if want is not None:
                assert T.route(r, which) == want and T.query(lib, r, which) == want, (r['name'], which)
    assert len({r['name'] for r in T.ROUTES}) == len(T.ROUTES)


FM_B = {1, 2, 3, 37, 4095, 4096, 4097, 8192, 8193, 131072, 131073, 524287, 524288, 524289, 2097151, 2097152, 2097153}
FM_D = sorted({d + o for d in (4, 8, 16, 32, 64, 128, 256) for o in (-1, 0, 1)} | {1, 2, 12, 24, 48, 96, 192, 260, 512, 1024})
IPNN_F = sorted({1, 2, 16, 17, 32, 33, 48, 49, 64, 65} | {r['F'] + o for r in T.ROUTES if r['op'] == 'ipnn' for o in (-1, 0, 1)} | {1170, 1171, 4000})
IPNN_D = (1, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 64, 65)
ATTN_D = sorted({d + o for d in (4, 8, 16, 32, 64, 128, 192, 256) for o in (-1, 0, 1)} | {1, 12, 20, 24, 48})


def _fm_sweep():
    for D in FM_D:
        # nchunk = B D / 4 at 524287 / 524288 / 524289 (where D divides), at multiples and non-multiples of 1024 above it, and small
        bs = set(FM_B) | {(n * 4) // D + o for n in (524287, 524288, 524289, 525312, 1048576, 2097152, 2098176) for o in (0, 1)}
        for B in sorted(b for b in bs if b >= 0):
            for F in (1, 5):
                for which in (0, 1):
                    for has_S in (0, 1):
                        yield which, B, F, D, has_S


def _ipnn_sweep():
    for F in IPNN_F:
        for D in IPNN_D:
            for B in (0, 1, 5, 65537, 0x7fffffff, 0x80000000):
                for which in (0, 1):
                    for mask in (0, 1):
                        yield which, B, F, D, mask


def _attn_sweep():
    for D in ATTN_D:
        for B in (0, 1, 5, 131073):
            for L in (0, 3):
                for which in (0, 1):
                    for mask in range(32 if which else 8):
                        yield which, B, L, D, mask


def test_mirror_matches_query_over_sweep():
    lib = _lib()
    assert {4, 5, 8, 12, 16, 17, 32, 33, 64, 65} <= set(IPNN_D) and {1, 2, 16, 17, 32, 33, 48, 49, 64, 65} <= set(IPNN_F)
    assert all(T.fm_vec_ok(d) and {d - 1, d + 1} <= set(FM_D) for d in (4, 8, 16, 32, 64, 128, 256)) and sum(map(T.fm_vec_ok, range(1, 2000))) == 7
    n = 0
    for a in _fm_sweep():
        assert lib.recnow_fm_route(*a) == T.fm_route(*a), a
        n += 1
    for a in _ipnn_sweep():
        assert lib.recnow_inner_pnn_route(*a) == T.ipnn_route(*a), a
        n += 1
    for a in _attn_sweep():
        assert lib.recnow_attention_dot_route(*a) == T.attn_route(*a), a
        n += 1
    assert n > 20000
    # the nchunk thresholds themselves, at D = 4 (nchunk = B)
    assert [T.fm_route(0, B, 2, 4, 1) // 100000 for B in (524287, 524288, 524289)] == [T.FM_VEC4, T.FM_WIDE, T.FM_WIDE]
    assert [T.fm_route(1, B, 2, 4, 1) // 100000 for B in (524287, 524288, 524289, 525312)] == [T.FM_VEC4, T.FM_WIDE, T.FM_VEC4, T.FM_WIDE]
    # empty calls, unsupported shapes, invalid arguments
    assert lib.recnow_fm_route(0, 0, 3, 16, 1) == 0 and lib.recnow_inner_pnn_route(0, 0, 3, 16, 0) == 0 and lib.recnow_attention_dot_route(1, 0, 3, 16, 0) == 0
    assert lib.recnow_inner_pnn_route(0, 5, 1, 16, 0) == 0 and lib.recnow_inner_pnn_route(1, 5, 1, 16, 0) == T.gen(16, 4)
    assert lib.recnow_inner_pnn_route(0, 5, 3, 65, 0) == T.EUNSUPPORTED and lib.recnow_inner_pnn_route(0, 5, 1171, 5, 0) == T.EUNSUPPORTED
    assert lib.recnow_inner_pnn_route(0, 5, 1170, 5, 0) == T.gen(8, 1) and lib.recnow_attention_dot_route(0, 5, 3, 257, 0) == T.EUNSUPPORTED
    assert T.EUNSUPPORTED not in (0, -1)
    for bad in ((2, 5, 3, 16, 1), (0, -1, 3, 16, 1), (0, 5, 0, 16, 1), (0, 5, 3, 0, 1), (0, 5, 3, 16, 2), (1, 5, 3, 16, 0)):
        assert lib.recnow_fm_route(*bad) == -1 == T.fm_route(*bad), bad
    for bad in ((2, 5, 3, 16, 0), (0, -1, 3, 16, 0), (0, 5, 0, 16, 0), (0, 5, 3, 0, 0), (0, 5, 3, 16, 2), (1, 5, 3, 16, -1)):
        assert lib.recnow_inner_pnn_route(*bad) == -1 == T.ipnn_route(*bad), bad
    for bad in ((2, 5, 3, 16, 0), (0, -1, 3, 16, 0), (0, 5, -1, 16, 0), (0, 5, 3, 0, 0), (0, 5, 3, 16, 8), (1, 5, 3, 16, 32), (1, 5, 3, 16, -1)):
        assert lib.recnow_attention_dot_route(*bad) == -1 == T.attn_route(*bad), bad


def test_table_reaches_every_reachable_code():
    reach = {op: set() for op in ('fm', 'ipnn', 'attn')}
    for a in _fm_sweep():
        reach['fm'].add((a[0], T.fm_route(*a)))
    for a in _ipnn_sweep():
        if a[1] <= 0x7fffffff:                                # beyond it a Gram shape runs the general kernels: no test can allocate that
            reach['ipnn'].add((a[0], T.ipnn_route(*a)))
    for a in _attn_sweep():
        reach['attn'].add((a[0], T.attn_route(*a)))
    have = {op: set() for op in reach}
    for r in T.ROUTES:
        have[r['op']].add((0, r['fwd']))
        if r['bwd'] is not None:
            have[r['op']].add((1, r['bwd']))
    # FM: SAVE_S is a template argument and lanes_per_row a run-time one -- every (family, SAVE_S) and every (family, lanes_per_row), not their product
    split = lambda cs: {(w, c // 1000, -1) for w, c in cs if c > 0} | {(w, c // 100000, c % 1000) for w, c in cs if c > 0}      # noqa: E731
    assert split(reach['fm']) == split(have['fm']), sorted(split(reach['fm']) ^ split(have['fm']))
    for op in ('ipnn', 'attn'):
        live = {c for c in reach[op] if c[1] > 0}
        missing = live - have[op]
        assert not missing, (op, sorted(missing))
        assert {c for c in have[op] if c[1] > 0} <= live, (op, sorted(have[op] - live))
    # what the sweep must have found, written out: every instantiation of the three ops
    fm_f = {(0, T.fm_code(T.FM_GENERIC, s, 0)) for s in (0, 1)} | {(0, T.fm_code(fam, s, l)) for fam in (T.FM_VEC4, T.FM_WIDE) for s in (0, 1)
                                                                   for l in (1, 2, 4, 8, 16, 32, 64)}
    fm_b = {(1, T.fm_code(T.FM_GENERIC, 0, 0))} | {(1, T.fm_code(fam, 0, l)) for fam in (T.FM_VEC4, T.FM_WIDE) for l in (1, 2, 4, 8, 16, 32, 64)}
    assert split(have['fm']) == split(fm_f | fm_b)
    gram_b = {(1, T.gram_b(D, nb, full, vec)) for D in (4, 8, 12, 16) for nb in (1, 2, 3, 4) for full in (0, 1) for vec in (0, 1)}
    gram_f = {(0, T.gram_f(D, two, vec)) for D in (4, 8, 12, 16) for two in (0, 1) for vec in (0, 1)}
    gen = {(w, T.gen(dm, wv)) for w in (0, 1) for dm in (8, 16, 32, 64) for wv in (4, 2, 1)}
    assert len(gram_b) == 64 and {c for c in have['ipnn'] if c[1] > 0} == gram_b | gram_f | gen
    assert {c for c in have['attn'] if c[1] > 0} == {(w, 200000 + c) for w in (0, 1) for c in (1, 2, 4, 8, 16)} | {(w, 100000 + g) for w in (0, 1) for g in (16, 32, 64)}
    assert all(T.inputs(r) <= 20e6 for r in T.ROUTES)


def test_every_loop_has_a_one_pass_and_a_ragged_multi_pass_row():
    """per kernel family with a grid-stride or row loop: a row with one pass, and a row with at least two whose last pass is ragged (B is no multiple
    of the pass).  k_fm_bwd_wide only ever sees whole workgroups: its multi-pass row ends on a whole workgroup short of a full pass."""
    seen = {}
    for r in T.ROUTES:
        g = T.geometry(r)
        for d in ('f', 'b'):
            e = g[d]
            if not e or not e['stride']:
                continue
            key = (r['op'], d, e['family']) + ((e.get('gs', 0),) if r['op'] == 'attn' else ())
            if r['op'] == 'fm' and e['family'] != T.FM_GENERIC:
                n, per = r['B'] * e['lanes'], e['cstride']
            else:
                n, per = r['B'], e['stride']
            seen.setdefault(key, set()).add('one' if n <= per else 'ragged' if n % per else 'whole')
    want = [('fm', 'f', T.FM_WIDE), ('fm', 'b', T.FM_WIDE), ('fm', 'b', T.FM_VEC4), ('fm', 'b', T.FM_GENERIC), ('ipnn', 'f', T.IPNN_GRAM_FWD),
            ('ipnn', 'b', T.IPNN_GRAM_BWD), ('ipnn', 'f', T.IPNN_GENERAL), ('ipnn', 'b', T.IPNN_GENERAL), ('attn', 'f', T.ATTN_V4, 0), ('attn', 'b', T.ATTN_V4, 0)]
    want += [('attn', d, T.ATTN_GENERIC, gs) for d in ('f', 'b') for gs in (16, 32, 64)]
    for key in want:
        assert {'one', 'ragged'} <= seen[key], (key, seen[key])
    assert seen[('fm', 'f', T.FM_VEC4)] == {'one'}            # its launcher never gives it 524288 chunks (the table's docstring)
    assert set(seen) == set(want) | {('fm', 'f', T.FM_VEC4)}


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------------------
def _close(a, ref):
    assert a.shape == ref.shape and np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


CLOSED = [dict(op='fm', name='closed fm', B=23, F=7, D=12, fwd=None, bwd=1, filter_neg=False, grads='both'),
          dict(op='ipnn', name='closed ipnn', B=23, F=7, D=5, fwd=None, bwd=1, filter_neg=False, grads='both')]
CLOSED += [dict(op='attn', name='closed attn %s %d' % (g, fn), B=23, F=6, D=9, fwd=None, bwd=1, filter_neg=bool(fn), grads=g)
           for g in ('both', 'dmat', 'dsum') for fn in (0, 1)]


@pytest.mark.parametrize('r', CLOSED, ids=[r['name'] for r in CLOSED])
def test_closed_form_is_the_autograd_oracle(r):
    d = C.random_data(r)
    if r['filter_neg']:
        assert C.score_clearance(d) >= C.CLEAR > C.KINK
    e, ref = C.compute(r, d, scales=True), C.oracle(r, d)
    for k in C.outputs(r):
        _close(e[k], ref[k])
        s = e['s_' + k][None] if (r['op'], k) == ('fm', 'dx') else e['s_' + k]
        assert (s >= np.abs(e[k]) - 1e-12).all(), k          # the scales are magnitudes of sums: each is at least the sum it belongs to


# ---- census ---------------------------------------------------------------------------------------------------------------------------------------------
IDS = [r['name'] for r in T.ROUTES]


@pytest.mark.parametrize('r', T.ROUTES, ids=IDS)
def test_census_is_exact(r):
    d, p = C.make(r)
    assert p == C.LADDER[0], 'the GPU test draws the first ladder entry'
    assert C.sums_exact(r, d) < C.EXACT
    assert all(C.same_bits(v, C.make(r, params=C.LADDER[0])[0][k]) for k, v in d.items())
    assert all((v != 0).all() for k, v in d.items() if k in ('x', 'u', 'doc'))
    e = C.exact(r, d)
    for k in C.outputs(r):
        assert (e[k] == np.rint(e[k])).all() and (not e[k].size or np.abs(e[k]).max() < C.EXACT), k
    # informative: rows differ from row to row, pair values from pair to pair, and the pinned rows carry gradient
    main = e[C.FORWARD[r['op']][0]].reshape(r['B'], -1)
    if r['B'] > 1 and main.shape[1] and not (r['op'] == 'fm' and r['F'] == 1) and r['F'] > 0:
        assert (np.abs(np.diff(main, axis=0)).sum(1) != 0).mean() > 0.9
    if r['op'] == 'ipnn' and r['F'] > 2:
        assert (np.diff(e['out'], axis=1) != 0).mean() > 0.8
    pinned = T.pinned_rows(r)
    strides = [g['stride'] for g in T.geometry(r).values() if g and g['stride']]
    assert {0, r['B'] - 1} <= set(pinned) and all(k in pinned for st in strides for k in range(0, r['B'], st))
    for k in ('g', 'dout', 'dmat', 'dsum'):
        if k in d and d[k].size:
            assert (d[k].reshape(r['B'], -1)[pinned] != 0).all(), k
    if C.has_bwd(r) and e[C.OUTPUTS[r['op']][-1]].size and not (r['op'] == 'fm' and r['F'] == 1) and r['F'] > 0:
        assert np.count_nonzero(e[C.OUTPUTS[r['op']][-1]]) > 0
    if T.inputs(r) <= 300000:
        ref = C.oracle(r, d)                                    # the exact values are the autograd oracle's (integers in fp64)
        if r['op'] == 'attn' and r['filter_neg']:
            # a raw score of exactly 0: the kernels pass no gradient there (C.attn), torch.clamp passes it -- du is compared at the other
            # positions and ddoc on the rows without such a position
            live = e['sraw'] != 0
            assert live.mean() > 0.8 and (ref['du'][live] == e['du'][live]).all() and (ref['ddoc'][live.all(1)] == e['ddoc'][live.all(1)]).all()
            assert (ref['mat'] == e['mat']).all() and (ref['ssum'] == e['ssum']).all()
        else:
            assert all((ref[k] == e[k]).all() for k in C.outputs(r))
    got = C.restate32(r, d)
    for k in C.outputs(r):
        assert got[k].dtype == np.float32 and C.same_bits(got[k], e[k]), '%s: the fp32 restatement of %s is not exact' % (r['name'], k)


# mistake -> (row, outputs it must change)
PLANTED = {
    'fm_tail_lane_stores': ('fm_wide_ragged_l64', ('y',)),
    'fm_remainder_dropped': ('fm_wide_ragged_l64', ('y', 'S', 'dx')),
    'fm_second_pass_skipped': ('fm_wide_two_pass', ('y', 'S', 'dx')),
    'fm_half_butterfly': ('fm_vec4_l8', ('y',)),
    'fm_prefetch_not_rotated': ('fm_wide_bwd_f9', ('dx',)),
    'ipnn_pair_base_off_by_row': ('ipnn_gram_d8_f17', ('out',)),
    'ipnn_g01_g11_dropped': ('ipnn_gram_d12_f33', ('out',)),
    'ipnn_field_ge_F_stored': ('ipnn_gram_d4_f15', ('out',)),
    'ipnn_UtX_missing': ('ipnn_gram_d16_f31', ('dx',)),
    'ipnn_prefetch_own_row': ('ipnn_gram_two_pass_vec', ('out', 'dx')),
    'attn_tail_pieces_counted': ('attn_v4_c1_nv63', ('mat', 'ssum')),
    'attn_filter_neg_passes_grad': ('attn_v4_c2_nv66', ('du', 'ddoc')),
    'attn_column_reduce_from_half': ('attn_v4_c4_nv68', ('mat', 'ddoc')),
    'attn_dsum_left_out': ('attn_d17', ('du', 'ddoc')),
}
# the same mistakes on a second family each, where the kernels differ
PLANTED_ALSO = {
    'fm_tail_lane_stores': ('fm_vec4_l16', ('y',)),
    'fm_remainder_dropped': ('fm_vec4_l4', ('y', 'S', 'dx')),
    'fm_second_pass_skipped': ('fm_wide_ragged_l2', ('dx',)),
    'fm_prefetch_not_rotated': ('fm_vec4_l32', ('dx',)),
    'ipnn_UtX_missing': ('ipnn_gen_d9', ('dx',)),
    'ipnn_prefetch_own_row': ('ipnn_gram_two_pass', ('out', 'dx')),
    'ipnn_pair_base_off_by_row': ('ipnn_gen_d17', ('out',)),
    'attn_filter_neg_passes_grad': ('attn_gs64_two_pass', ('du', 'ddoc')),
    'attn_dsum_left_out': ('attn_v4_dsum_only', ('du', 'ddoc')),
}
ALL_MISTAKES = [m for op in C.MISTAKES for m in C.MISTAKES[op]]


@pytest.mark.parametrize('mistake', ALL_MISTAKES)
def test_census_has_teeth(mistake):
    """an fp32 restatement of the kernels with one planted mistake is NOT bit-equal to the census"""
    assert set(PLANTED) == set(ALL_MISTAKES) and len(ALL_MISTAKES) == 14
    for table in (PLANTED, PLANTED_ALSO):
        if mistake not in table:
            continue
        name, changed = table[mistake]
        r = T.BY_NAME[name]
        assert mistake in C.MISTAKES[r['op']]
        d, _ = C.make(r, params=C.LADDER[0])
        e = C.exact(r, d)
        ok = C.restate32(r, d)
        assert all(C.same_bits(ok[k], e[k]) for k in C.outputs(r))
        bad = C.restate32(r, d, mistake=mistake)
        for k in changed:
            assert not C.same_bits(bad[k], e[k]), '%s on %s: %s is still bit-equal' % (mistake, name, k)


WORST = {}


@pytest.mark.parametrize('r', T.ROUTES, ids=IDS)
def test_fp32_restatement_under_half_the_bound(r):
    d = C.random_data(r)
    if r['op'] == 'attn' and r['filter_neg']:
        assert C.score_clearance(d) >= C.CLEAR > C.KINK
    ref = C.compute(r, d, scales=True)
    m = C.margins(r, C.restate32(r, d), ref, ref)
    for k, v in m.items():
        WORST[(r['op'], k)] = max(WORST.get((r['op'], k), 0.0), v)
    assert max(m.values()) <= 0.5, m


def test_worst_restatement_margins_are_reported():
    print('largest fraction of the bound in the fp32 restatement: ' + '  '.join('%s.%s %.4f' % (op, k, v) for (op, k), v in sorted(WORST.items())))
    assert all(v <= 0.5 for v in WORST.values())


# ---- the alignment helper -------------------------------------------------------------------------------------------------------------------------------
class _Stand:
    """a stand-in for a tensor with a chosen address"""
    copies = 0

    def __init__(self, ptr):
        self._ptr = ptr

    def data_ptr(self):
        return self._ptr

    def clone(self):
        _Stand.copies += 1
        return _Stand(0x7000_0000 + 256 * _Stand.copies)


def test_aligned_fields_copies_exactly_the_misaligned_fields_of_a_vector_route():
    from rec_now_amd import _lib
    base = 0x10000
    fields = [_Stand(base), _Stand(base + 4), _Stand(base + 16), _Stand(base + 8), _Stand(base + 12), _Stand(base + 4096)]
    _Stand.copies = 0
    same = _lib.aligned_fields(fields, False)
    assert isinstance(same, list) and all(a is b for a, b in zip(same, fields)) and _Stand.copies == 0      # a scalar route: nothing is touched
    out = _lib.aligned_fields(tuple(fields), True)
    assert isinstance(out, list) and len(out) == len(fields)
    assert [a is b for a, b in zip(out, fields)] == [True, False, True, False, False, True] and _Stand.copies == 3
    assert all(t.data_ptr() % 16 == 0 for t in out)
    assert [t.data_ptr() for t in fields] == [base, base + 4, base + 16, base + 8, base + 12, base + 4096]      # the caller's tensors are not changed
    # a real contiguous view one float into a buffer (on the host: only the address arithmetic is under test)
    buf = torch.arange(41, dtype=torch.float32)
    view = buf[1:].view(5, 8)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    got = _lib.aligned_fields([buf[:40].view(5, 8), view], True)
    assert got[0].data_ptr() == buf.data_ptr() and got[1].data_ptr() % 16 == 0 and torch.equal(got[1], view)

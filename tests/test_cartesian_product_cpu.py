"""CPU: CartesianProductLayer's host route against the reference's own goldens, the limits of the GPU route (checked on the host before any
launch), and the host twins of the crossed-id kernels -- recnow_cross_text_host / recnow_cross_hash_ids_host run the very code the kernels
compile (csrc/hash64.hpp: composer, matcher, hashes) -- against the plain-Python oracle of tests/_cross_oracle.py.  No kernel is launched.

The limit "worst-case text at most 96 bytes" has no test of its own: with at most 4 inputs of at most 20 bytes and a separator of at most 4 bytes
the longest text is 92 bytes, so the other limits keep it from being reached (the 92-byte case is composed and hashed below)."""
import itertools

import numpy as np
import pytest
import torch

import _cross_oracle as C
import _hash_oracle as O

I32_MIN, I64_MIN, I64_MAX = -(1 << 31), -(1 << 63), (1 << 63) - 1
EDGE_IDS = [0, 9, 10, -1, 10 ** 9 - 1, 10 ** 9, -10 ** 9, 10 ** 18, I32_MIN, I64_MIN, I64_MAX]
EDGE_IDS_32 = [v for v in EDGE_IDS if I32_MIN <= v < (1 << 31)]
SEPARATORS = ['', '-', '_x', 'ab_c']


def layer(separator='-'):
    from rec_now_amd.layers import CartesianProductLayer
    return CartesianProductLayer(separator=separator)


def crossed(arrays, separator='-', patterns=None, default=''):
    """CrossedIds over HOST tensors: construction checks the limits and launches nothing; its descriptor then holds host pointers."""
    from rec_now_amd.layers import CrossedIds
    return CrossedIds([torch.from_numpy(np.ascontiguousarray(a)) for a in arrays], separator, patterns, default)


def host_texts(cr):
    """(B, P) object array of bytes through recnow_cross_text_host."""
    from rec_now_amd import _lib
    B, P = cr.shape
    W = max(8, -(-cr.longest_bytes // 8) * 8)
    text = np.full((B, P, W), 0xee, dtype=np.uint8)
    lens = np.full((B, P), -7, dtype=np.int32)
    rc = _lib.load().recnow_cross_text_host(cr.desc(), B, W, text.ctypes.data, lens.ctypes.data)
    assert rc == 0
    out = np.empty((B, P), dtype=object)
    for b in range(B):
        for j in range(P):
            n = lens[b, j]
            assert 0 <= n <= W and not text[b, j, n:].any(), 'not zero padded'
            out[b, j] = text[b, j, :n].tobytes()
    return out


def host_buckets(cr, num_bins, num_hash, salts, first_unsalted, default_buckets=None):
    from rec_now_amd import _lib
    B, P = cr.shape
    sl = np.array(O.expand_salts(salts, num_hash), dtype=np.int64)
    out = np.full((B, P, num_hash), -7, dtype=np.int64)
    rc = _lib.load().recnow_cross_hash_ids_host(cr.desc(default_buckets), B, sl.ctypes.data, num_hash, int(first_unsalted), num_bins, out.ctypes.data)
    return rc, out


def same(a, b):
    return a.shape == b.shape and a.tolist() == b.tolist()


# ---- 1. host route -------------------------------------------------------------------------------------------------------------------------
def test_host_route_meets_the_reference_goldens(golden):
    g = golden('cartesian')
    prod = [g['prod_in1'], g['prod_in2'], g['prod_in3']]
    out = layer()(prod)
    assert out.dtype == object and same(out, g['prod_plain'].astype(object))
    pats = [p.decode() for p in g['prod_patterns']]
    assert pats == ['A', 'f', 'None']
    assert same(layer()(prod, invalid_pattern_list=pats, default_result_str=''), g['prod_invalid'].astype(object))
    # lists, and an integer tensor moved to the host
    assert same(layer()([g['prod_in1'].tolist(), [[s.decode() for s in r] for r in g['prod_in2']], torch.from_numpy(g['prod_in3'])]),
                g['prod_plain'].astype(object))
    assert same(layer()([g['bcast_in1'], g['bcast_in2'], g['bcast_in3']]), g['bcast_out'].astype(object))
    digits = layer('')([g['digits_in1'], g['digits_in2'], g['digits_in3']])
    assert np.array_equal(np.array([[float(v) for v in r] for r in digits], dtype=np.float32), g['digits_out'])
    # the seven pattern / result pairs: the four joined strings as two fields each
    left, right = zip(*[s.split(b'-') for s in g['pat_input']])
    fields = [np.array(left, dtype=object).reshape(4, 1), np.array(right, dtype=object).reshape(4, 1)]
    assert [a + b'-' + b for a, b in zip(left, right)] == g['pat_input'].tolist()
    for pat, none, want in zip(g['pat'], g['pat_none'], g['pat_out']):
        pl = [None if n else p.decode() for p, n in zip(pat, none)]
        assert layer()(fields, invalid_pattern_list=pl).reshape(-1).tolist() == want.tolist(), pl
        assert C.texts(fields, '-', pl).reshape(-1).tolist() == want.tolist(), pl          # and the oracle meets them too


def test_host_route_every_input_one_row():
    out = layer()([[['A', 'B']], 'a', np.array([[3, 4]])])
    assert out.shape == (1, 4) and out.tolist() == [[b'A-a-3', b'A-a-4', b'B-a-3', b'B-a-4']]
    cr = crossed([np.array([[1, 2]]), np.array(7)])
    assert cr.shape == (1, 2) and host_texts(cr).tolist() == [[b'1-7', b'2-7']]


def test_wrong_number_of_patterns():
    with pytest.raises(ValueError, match='length not equal'):
        layer()([['a'], ['b']], invalid_pattern_list=['a'])
    with pytest.raises(ValueError, match='length not equal'):
        crossed([np.array([1]), np.array([2])], patterns=['a', None, None])


def test_floats_are_refused():
    for bad in (torch.zeros(2, 2), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(TypeError, match='crosses ids'):
            layer()([bad, torch.zeros(2, dtype=torch.int64)])
    with pytest.raises(TypeError, match='crosses ids'):
        layer()([[1.5], ['a']])


# ---- 2. the limits of the GPU route, one test each -------------------------------------------------------------------------------------------
def test_limit_inputs():
    with pytest.raises(NotImplementedError, match='at most 4 inputs'):
        crossed([np.array([1])] * 5)


def test_limit_separator():
    with pytest.raises(NotImplementedError, match='at most 4 bytes'):
        crossed([np.array([1]), np.array([2])], separator='-----')
    assert crossed([np.array([1]), np.array([2])], separator='éé').separator == b'\xc3\xa9\xc3\xa9'      # 4 bytes of utf-8


def test_limit_default_string():
    with pytest.raises(NotImplementedError, match='at most 96 bytes'):
        crossed([np.array([1]), np.array([2])], patterns=['1', None], default='x' * 97)


def test_limit_entries():
    from rec_now_amd.layers import MultiHashLayer
    cr = crossed([np.zeros((1 << 22, 1), dtype=np.int32), np.zeros((1, 32), dtype=np.int32), np.zeros((1, 32), dtype=np.int32)])
    assert cr.shape == (1 << 22, 1024)
    with pytest.raises(NotImplementedError, match='fewer than 2\\^31'):
        MultiHashLayer(100, 8, num_hash=1)(cr)


def test_limit_unsalted_hash_takes_32_bytes():
    from rec_now_amd.layers import FastMultiHashLayer, MultiHashLayer
    i32, i64 = np.zeros((2, 2), dtype=np.int32), np.zeros((2, 2), dtype=np.int64)
    for arrays, kw in (([i64, i64], {}), ([i32, i64], dict(separator='--')), ([i32, i32], dict(patterns=['1', None], default='x' * 33)),
                       ([i32, i32], dict(default='x' * 33))):
        with pytest.raises(NotImplementedError, match='up to 32 bytes'):
            FastMultiHashLayer(100, -1)(crossed(arrays, **kw))
    # two int32 inputs always pass, int32 x int64 under '-' is exactly 32 bytes (and then meet the GPU requirement: these tensors are on the host), as does every cross under MultiHashLayer
    for lay, cr in ((FastMultiHashLayer(100, -1), crossed([i32, i32], separator='ab_c')), (FastMultiHashLayer(100, -1), crossed([i32, i64])),
                    (MultiHashLayer(100, -1), crossed([i64] * 4, 'ab_c'))):
        with pytest.raises(RuntimeError, match='only on the GPU'):
            lay(cr)


def test_limit_patterns():
    two = [np.array([1]), np.array([2])]
    with pytest.raises(NotImplementedError, match='at most 8 alternatives'):
        crossed(two, patterns=['|'.join('abcdefghi'), None])
    with pytest.raises(NotImplementedError, match='at most 24 bytes'):
        crossed(two, patterns=[None, 'x' * 25])
    for bad in ('a.*', '[0-9]', 'a+', '(a)', 'a\\d', '^a'):
        with pytest.raises(NotImplementedError, match='host route'):
            crossed(two, patterns=[bad, None])
    with pytest.raises(NotImplementedError, match='host route'):
        crossed(two, separator='.', patterns=['a', None])
    assert crossed(two, separator='.', patterns=None).spec is None          # without patterns any separator is a literal


# ---- 3. the host twins: texts and buckets ---------------------------------------------------------------------------------------------------
def _id_of_len(n):
    """An int64 whose decimal text has n bytes, 1 <= n <= 20."""
    return int('1234567890123456789'[:n]) if n < 20 else -1234567890123456789


def _cases():
    """(name, arrays) -- 1 to 4 inputs, int32 / int64 mixed, one-row inputs, the edge ids, and pairs whose joined length takes every value."""
    e64, e32 = np.array(EDGE_IDS, dtype=np.int64), np.array(EDGE_IDS_32, dtype=np.int32)
    pairs = [(la, lb) for la in range(1, 21) for lb in sorted({1, la, 20, 21 - la})]
    lengths = np.array([[_id_of_len(la), _id_of_len(lb)] for la, lb in pairs], dtype=np.int64)
    return [
        ('one', [e64.reshape(1, -1)]),
        ('one32', [e32]),
        ('edges', [np.tile(e64, (2, 1)), np.tile(e32, (2, 1))]),
        ('edges row', [e32.reshape(1, -1), np.stack([e64, e64[::-1]])]),
        ('three', [e32[:3].reshape(3, 1), e64[:9].reshape(3, 3), np.array([[7, -8]], dtype=np.int32)]),
        ('four', [np.array([[I64_MIN, 5]] * 2, dtype=np.int64), np.array([[I64_MIN], [1]], dtype=np.int64), np.array([I64_MIN, I64_MAX], dtype=np.int64),
                  np.array([[[I64_MIN], [0]]] * 2, dtype=np.int64)]),
        ('lengths', [lengths[:, :1], lengths[:, 1:]]),
    ]


CASES = _cases()


def test_cases_cover_every_length_and_the_longest_text():
    lens = set()
    for sep in ('', '-'):
        lens |= {len(t) for t in C.texts(dict(CASES)['lengths'], sep).reshape(-1)}
    assert lens >= set(range(2, 42)), sorted(set(range(2, 42)) - lens)
    assert max(len(t) for t in C.texts(dict(CASES)['four'], 'ab_c').reshape(-1)) == 92


@pytest.mark.parametrize('sep', SEPARATORS)
def test_text_host_equals_the_python_composition(sep):
    for name, arrays in CASES:
        cr = crossed(arrays, sep)
        want = C.texts(arrays, sep)
        assert cr.shape == want.shape, name
        assert same(host_texts(cr), want), (name, sep)


@pytest.mark.parametrize('sep', SEPARATORS)
def test_hash_ids_host_equals_the_oracle(sep):
    for name, arrays in CASES:
        cr = crossed(arrays, sep)
        want_texts = C.texts(arrays, sep)
        for salts, nh in ((1, 2), ([9, 2, 77], 3)):                                     # MultiHashLayer: every hash salted
            for num_bins in (1000, (1 << 63) - 1):
                rc, got = host_buckets(cr, num_bins, nh, salts, False)
                assert rc == 0 and np.array_equal(got, C.buckets(want_texts, num_bins, nh, salts, False)), (name, sep, salts, num_bins)
        rc, got = host_buckets(cr, 1000, 2, 1, True)                                    # FastMultiHashLayer: hash 0 unsalted, texts of <= 32 bytes
        if cr.longest_bytes <= 32:
            assert rc == 0 and np.array_equal(got, C.buckets(want_texts, 1000, 2, 1, True)), (name, sep)
        else:
            assert rc == -3 and (got == -7).all(), (name, sep)                          # RECNOW_EUNSUPPORTED, nothing written


def test_unsalted_hash_on_texts_of_up_to_32_bytes():
    """Two int32 inputs: every length from 3 ("0-0") to 26 under the 4-byte separator, the 16 / 17 byte edge of Fingerprint64 included."""
    vals = [0, -1, 10, -10, 999, -9999, 12345, 123456, -1234567, 12345678, 123456789, I32_MIN, (1 << 31) - 1]
    a = np.array(vals, dtype=np.int32)
    arrays = [a.reshape(-1, 1), a.reshape(1, -1)]
    seen = set()
    for sep in SEPARATORS:
        want_texts = C.texts(arrays, sep)
        seen |= {len(t) for t in want_texts.reshape(-1)}
        rc, got = host_buckets(crossed(arrays, sep), 1 << 20, 3, 5, True)
        assert rc == 0 and np.array_equal(got, C.buckets(want_texts, 1 << 20, 3, 5, True)), sep
    assert seen >= set(range(2, 27))


def test_host_entries_refuse_bad_descriptors():
    from rec_now_amd import _lib
    lib = _lib.load()
    cr = crossed([np.array([1, 2]), np.array([3, 4])], patterns=['1', None], default='d')
    sl = np.array([1, 2], dtype=np.int64)
    out = np.zeros((2, 1, 2), dtype=np.int64)
    hash_rc = lambda d, nb=10: lib.recnow_cross_hash_ids_host(d, 2, sl.ctypes.data, 2, 0, nb, out.ctypes.data)      # noqa: E731
    assert hash_rc(cr.desc([3, 4])) == 0
    assert hash_rc(cr.desc([3, 10])) == -1                                   # a default bucket outside the table
    for field, value in (('n_inputs', 5), ('n_inputs', 0), ('sep_len', 5), ('default_len', 97)):
        d = cr.desc([3, 4])
        setattr(d, field, value)
        assert hash_rc(d) == -1, field
    d = cr.desc([3, 4])
    d.n_alt[0] = 9
    assert hash_rc(d) == -1
    d = cr.desc([3, 4])
    d.lit_len[0][0] = 25
    assert hash_rc(d) == -1
    d = cr.desc([3, 4])
    d.dtype[1] = 7
    assert hash_rc(d) == -1
    text, lens = np.zeros((2, 1, 48), dtype=np.uint8), np.zeros((2, 1), dtype=np.int32)
    assert lib.recnow_cross_text_host(cr.desc(), 2, 48, text.ctypes.data, lens.ctypes.data) == 0
    assert lib.recnow_cross_text_host(cr.desc(), 2, 40, text.ctypes.data, lens.ctypes.data) == -1      # narrower than the longest text (41)
    assert lib.recnow_cross_text_host(cr.desc(), 2, 44, text.ctypes.data, lens.ctypes.data) == -1      # not whole words


# ---- 4. the matcher, exhaustively over a small space, against `re` ----------------------------------------------------------------------------
MATCH_IDS = np.array([-11, -1, 0, 1, 11], dtype=np.int64)
LITERALS = ['', '1', '-1', '11', '1-1', '-']
PATTERNS = LITERALS + [a + '|' + b for a, b in itertools.permutations(LITERALS, 2)]
DEFAULT = 'DEF!'


@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('sep', ['-', '--', '_'])
def test_matcher_is_the_regular_expressions_own_match(n, sep):
    """Every element of every cross is compared: the replaced text through recnow_cross_text_host, the buckets through recnow_cross_hash_ids_host."""
    arrays = [MATCH_IDS.reshape(1, -1)] * n
    plain = C.texts(arrays, sep)
    dflt_bk = O.buckets([DEFAULT.encode()], 1000, 2, 1, False)[0].tolist()
    plain_bk = C.buckets(plain, 1000, 2, 1, False)
    replaced = 0
    for pos in range(n):
        for pat in PATTERNS:
            pl = [None] * n
            pl[pos] = pat
            want = C.texts(arrays, sep, pl, DEFAULT)
            cr = crossed(arrays, sep, pl, DEFAULT)
            got = host_texts(cr)
            assert same(got, want), (sep, pl, [(g, w, p) for g, w, p in zip(got.reshape(-1), want.reshape(-1), plain.reshape(-1)) if g != w][:5])
            hit = np.array([w != p for w, p in zip(want.reshape(-1), plain.reshape(-1))]).reshape(want.shape)
            replaced += int(hit.sum())
            rc, bk = host_buckets(cr, 1000, 2, 1, False, dflt_bk)
            assert rc == 0 and np.array_equal(bk, np.where(hit[..., None], np.array(dflt_bk), plain_bk)), (sep, pl)
    assert replaced > 0
    # patterns on every input at once
    pl = ['1|-1', '', '11'][:n]
    assert same(host_texts(crossed(arrays, sep, pl, DEFAULT)), C.texts(arrays, sep, pl, DEFAULT))


def test_matcher_reads_the_joined_text_not_the_fields():
    """Fields 5 and -1 under '-' join to "5--1", which the reference's ^.*-(1)$ matches although the second field is not "1"."""
    arrays = [np.array([[5]]), np.array([[-1, 1, 2]])]
    assert C.texts(arrays, '-', [None, '1'], 'X').tolist() == [[b'X', b'X', b'5-2']]
    assert host_texts(crossed(arrays, '-', [None, '1'], 'X')).tolist() == [[b'X', b'X', b'5-2']]
    assert layer()(arrays, invalid_pattern_list=[None, '1'], default_result_str='X').tolist() == [[b'X', b'X', b'5-2']]

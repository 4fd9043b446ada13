"""CPU: the hash functions of MultiHashLayer / FastMultiHashLayer and the host side of both layers.  No kernel is launched: the C entry
points recnow_hash_ids_host / recnow_hash_bytes_host run the very code the kernels compile (csrc/hash64.hpp) on the host."""
import ctypes

import numpy as np
import pytest
import torch

import _hash_oracle as O

SUM_ABS_BOUND = 1e-5          # the reference tests' own bound: sum of absolute differences


def _ids_sets():
    edge = []
    for k in range(1, 19):
        edge += [10 ** k - 1, 10 ** k, 10 ** k + 1]
    edge += [-v for v in edge]
    edge += [0, -1, -(1 << 31), (1 << 31) - 1, -(1 << 63), (1 << 63) - 1]
    rng = np.random.default_rng(11)
    return {
        'golden': np.arange(1, 15, dtype=np.int64),
        'edges': np.array(edge, dtype=np.int64),
        'wide': rng.integers(-(1 << 63), (1 << 63) - 1, 100000, dtype=np.int64, endpoint=True),
        'narrow': rng.integers(0, 1 << 20, 100000, dtype=np.int64),
    }


IDS = _ids_sets()
NUM_BINS = [1, 2, 3, 1000, (1 << 31) - 1, 1 << 31, (1 << 63) - 1]


def host_hash_ids(ids, num_bins, num_hash, salts, first_unsalted):
    from rec_now_amd import _lib
    from rec_now_amd.layers.multi_hash_layer import expand_salts
    lib = _lib.load()
    ids = np.ascontiguousarray(ids)
    sl = np.array(expand_salts(salts, num_hash), dtype=np.int64)
    out = np.full((ids.size, num_hash), -7, dtype=np.int64)
    rc = lib.recnow_hash_ids_host(ids.ctypes.data, 2 if ids.dtype == np.int32 else 3, ids.size, sl.ctypes.data, num_hash, int(first_unsalted),
                                  num_bins, out.ctypes.data)
    assert rc == 0
    return out


def host_hash_bytes(strs, num_bins, num_hash, salts, first_unsalted):
    from rec_now_amd import _lib
    lib = _lib.load()
    off = np.zeros(len(strs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strs], out=off[1:])
    buf = np.frombuffer(b''.join(strs) + b'\0', dtype=np.uint8).copy()
    sl = np.array(O.expand_salts(salts, num_hash), dtype=np.int64)
    out = np.full((len(strs), num_hash), -7, dtype=np.int64)
    rc = lib.recnow_hash_bytes_host(buf.ctypes.data, off.ctypes.data, len(strs), sl.ctypes.data, num_hash, int(first_unsalted), num_bins,
                                    out.ctypes.data)
    return rc, out


# ---- 1. the oracle against published / recorded vectors ----------------------------------------------------------------------------------
def test_oracle_reproduces_the_reference_literals(golden):
    """All 84 bucket literals of the reference's two *_no_emb tests (texts of 1 and 2 bytes: salts 1, 2, 3, and unsalted + salts 2, 3)."""
    g = golden('multi_hash')
    ids = g['int_inputs']
    nb, nh, salts = int(g['num_bins_no_emb']), int(g['num_hash']), int(g['salts'])
    assert np.array_equal(O.layer_call('multi', ids, nb, nh, salts, None, 'concat'), g['multi_no_emb'])
    assert np.array_equal(O.layer_call('fast', ids, nb, nh, salts, None, 'concat'), g['fast_no_emb'])
    assert g['multi_no_emb'].size + g['fast_no_emb'].size == 84


def test_oracle_siphash_paper_vector():
    """SipHash-2-4 reference paper, appendix A: key 00..0f, message 00..0e."""
    k0 = int.from_bytes(bytes(range(8)), 'little')
    k1 = int.from_bytes(bytes(range(8, 16)), 'little')
    assert O.siphash24(k0, k1, bytes(range(15))) == 0xa129ca6149be45e5


def test_oracle_recalled_tensorflow_doc_examples():
    """Examples of the TensorFlow API documentation (keras Hashing, tf.strings.to_hash_bucket_fast / _strong), RECALLED FROM MEMORY: the
    documentation is not part of this repository.  With the reference goldens above (Fingerprint64 at lengths 1 and 2) these are all that pins
    Fingerprint64 at lengths 3..16: three values modulo 3, at lengths 3, 5 and 10.  Lengths 17..32 are pinned by nothing TensorFlow-derived
    (see rec_now_amd/layers/multi_hash_layer.py)."""
    assert [O.bucket(c.encode(), None, 3) for c in 'ABCDE'] == [1, 0, 1, 1, 2]
    assert [O.siphash24(133, 137, c.encode()) % 3 for c in 'ABCDE'] == [1, 2, 1, 0, 2]
    assert [O.bucket(s, None, 3) for s in (b'Hello', b'TensorFlow', b'2.x')] == [0, 2, 2]
    assert [O.siphash24(1, 2, s) % 3 for s in (b'Hello', b'TF')] == [2, 0]


def test_oracle_vector_and_scalar_forms_agree():
    rng = np.random.default_rng(3)
    strs = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in range(0, 33) for _ in range(3)]
    got = O.buckets(np.array(strs, dtype=object), 1000003, 3, [9, 4], True)
    for i, s in enumerate(strs):
        assert got[i].tolist() == [O.bucket(s, None, 1000003), O.bucket(s, 4, 1000003), O.bucket(s, 5, 1000003)]


# ---- 2. the library's host entry points, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize('first_unsalted', [False, True])
@pytest.mark.parametrize('name', sorted(IDS))
def test_hash_ids_host_equals_oracle(name, first_unsalted):
    ids = IDS[name]
    for num_bins in NUM_BINS:
        got = host_hash_ids(ids, num_bins, 4, 1, first_unsalted)
        assert np.array_equal(got, O.buckets(ids, num_bins, 4, 1, first_unsalted)), (name, num_bins)
    for num_hash in (1, 2, 3):
        for salts in (7, [3, 11], [0, (1 << 62) + 5]):
            got = host_hash_ids(ids[:2000], 1000, num_hash, salts, first_unsalted)
            assert np.array_equal(got, O.buckets(ids[:2000], 1000, num_hash, salts, first_unsalted)), (name, num_hash, salts)


@pytest.mark.parametrize('first_unsalted', [False, True])
def test_hash_ids_host_int32(first_unsalted):
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(-(1 << 31), (1 << 31) - 1, 20000, endpoint=True), [0, -1, -(1 << 31), (1 << 31) - 1]]).astype(np.int32)
    for num_bins in (3, 1000, 1 << 31):
        assert np.array_equal(host_hash_ids(ids, num_bins, 3, 1, first_unsalted), O.buckets(ids.astype(np.int64), num_bins, 3, 1, first_unsalted))


def test_hash_bytes_host_equals_oracle_and_refuses_long_unsalted_inputs():
    rng = np.random.default_rng(7)
    short = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in range(0, 33) for _ in range(4)]
    for fu in (False, True):
        for num_bins in (3, 1000, (1 << 63) - 1):
            rc, got = host_hash_bytes(short, num_bins, 3, [5, 6, 7], fu)
            assert rc == 0
            assert np.array_equal(got, O.buckets(np.array(short, dtype=object), num_bins, 3, [5, 6, 7], fu))
    longer = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in range(33, 101)]
    rc, got = host_hash_bytes(longer, 1000, 3, [5, 6, 7], False)                # SipHash: any length
    assert rc == 0
    assert np.array_equal(got, O.buckets(np.array(longer, dtype=object), 1000, 3, [5, 6, 7], False))
    rc, _ = host_hash_bytes(longer[:1], 1000, 3, [5, 6, 7], True)               # Fingerprint64 past 32 bytes: an error code, never a bucket
    assert rc == -3
    from rec_now_amd.layers.multi_hash_layer import hash_strings_host
    with pytest.raises(NotImplementedError, match='33 bytes'):
        hash_strings_host(['x' * 33], 1000, [1, 2], True)
    assert hash_strings_host(['x' * 33], 1000, [1, 2], False).shape == (1, 2)


def test_hash_host_rejects_bad_arguments():
    from rec_now_amd import _lib
    lib = _lib.load()
    ids = np.arange(4, dtype=np.int64)
    out = np.zeros((4, 2), dtype=np.int64)
    ok = np.array([1, 2], dtype=np.int64)
    neg = np.array([1, -2], dtype=np.int64)
    call = lambda sl, nh, nb, dt=3: lib.recnow_hash_ids_host(ids.ctypes.data, dt, 4, sl.ctypes.data, nh, 0, nb, out.ctypes.data)      # noqa: E731
    assert call(ok, 2, 10) == 0
    assert call(neg, 2, 10) == -1
    assert call(ok, 0, 10) == -1
    assert call(ok, 2, 0) == -1
    assert call(ok, 2, 10, dt=0) == -1


# ---- 3. the reference goldens through the oracle -----------------------------------------------------------------------------------------
def test_reference_goldens_through_the_oracle(golden):
    g = golden('multi_hash')
    strs = [[s.decode() for s in row] for row in g['str_inputs']]
    nb, nh, salts = int(g['num_bins_emb']), int(g['num_hash']), int(g['salts'])
    w = np.full((3, 2), float(g['pooling_weight']))
    mt, ft = [t.astype(np.float64) for t in g['multi_tables']], g['fast_table'].astype(np.float64)
    diff = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - b).sum())      # noqa: E731
    assert diff(O.layer_call('multi', strs, nb, nh, salts, mt, 'concat'), g['multi_concat']) < SUM_ABS_BOUND
    assert diff(O.layer_call('multi', strs, nb, nh, salts, mt, 'sum'), g['multi_sum']) < SUM_ABS_BOUND
    assert diff(O.layer_get_pooling('multi', strs, nb, nh, salts, mt, w), g['multi_pooling']) < SUM_ABS_BOUND
    assert diff(O.layer_call('fast', strs, nb, nh, salts, ft, 'concat'), g['fast_concat']) < SUM_ABS_BOUND
    assert diff(O.layer_call('fast', strs, nb, nh, salts, ft, 'sum'), g['fast_sum']) < SUM_ABS_BOUND
    assert diff(O.layer_get_pooling('fast', strs, nb, nh, salts, ft, w), g['fast_pooling']) < SUM_ABS_BOUND
    nbn = int(g['num_bins_no_emb'])
    assert diff(O.layer_call('multi', g['int_inputs'], nbn, nh, salts, None, 'concat'), g['multi_no_emb']) < SUM_ABS_BOUND
    assert diff(O.layer_call('fast', g['int_inputs'], nbn, nh, salts, None, 'concat'), g['fast_no_emb']) < SUM_ABS_BOUND


# ---- 4. host side of the layers ----------------------------------------------------------------------------------------------------------
def _layers():
    from rec_now_amd.layers import FastMultiHashLayer, MultiHashLayer
    return {'multi': MultiHashLayer, 'fast': FastMultiHashLayer}


def test_layers_are_exported():
    import rec_now_amd.layers as L
    assert L.MultiHashLayer.__name__ == 'MultiHashLayer' and L.FastMultiHashLayer.__name__ == 'FastMultiHashLayer'


def test_salts_expansion():
    for cls in _layers().values():
        assert cls(10, num_hash=3, salts=1).salts == [1, 2, 3]
        assert cls(10, num_hash=4, salts=[5, 9]).salts == [5, 9, 10, 11]
        assert cls(10, num_hash=2, salts=(7, 3, 1)).salts == [7, 3, 1]
        assert cls(10).salts == [1, 2] and cls(10).num_hash == 2 and cls(10).embedding_dim == -1


def test_validation_errors():
    for cls in _layers().values():
        with pytest.raises(ValueError, match='num_bins'):
            cls(0)
        with pytest.raises(ValueError, match='num_hash'):
            cls(10, num_hash=0)
        with pytest.raises(ValueError, match='salts'):
            cls(10, salts=-1)
        with pytest.raises(ValueError, match='salts'):
            cls(10, num_hash=2, salts=[3, -3])
        with pytest.raises(NotImplementedError, match='num_hash'):
            cls(10, num_hash=17)
        with pytest.raises(ValueError, match='2\\^31'):
            cls(1 << 30, 4, num_hash=2)
        with pytest.raises(TypeError, match='unexpected keyword'):
            cls(10, bogus=1)
        layer = cls(10, 4)
        with pytest.raises(TypeError, match='integer ids'):
            layer(torch.zeros(3, 2))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            layer(torch.zeros(3, 2, dtype=torch.int64))
        with pytest.raises(TypeError, match='no CPU fallback'):
            layer([[1, 2], [3, 4]])
        with pytest.raises(ValueError, match='embedding_dim'):
            cls(10).get_pooling([['a']])


def test_table_shapes_and_names():
    multi, fast = _layers()['multi'](10, 4, num_hash=3, name='age'), _layers()['fast'](10, 4, num_hash=3, name='age')
    for layer in (multi, fast):
        layer._build_device = torch.device('cpu')
        layer.build()
    w = multi.named_weights()
    assert sorted(w) == ['embedding_layers/%d/embeddings' % i for i in range(3)]
    assert all(tuple(v.shape) == (10, 4) for v in w.values())
    w = fast.named_weights()
    assert sorted(w) == ['embedding_layer/embeddings'] and tuple(w['embedding_layer/embeddings'].shape) == (30, 4)
    for layer in (multi, fast):                                     # default initializer: uniform in [-1e-4, 1e-4]
        for v in layer.named_weights().values():
            assert 0 < float(v.detach().abs().max()) <= 1e-4 and v.requires_grad
    frozen = _layers()['fast'](10, 4, trainable=False)
    frozen._build_device = torch.device('cpu')
    frozen.build()
    assert not frozen.tables[0].requires_grad
    none = _layers()['multi'](10)
    none.build()
    assert none.named_weights() == {}


@pytest.mark.parametrize('kind', ['multi', 'fast'])
def test_output_shapes_against_the_oracle(kind):
    """Every (embedding or not, number of hash functions, combiner, input rank) against the shapes the oracle's restatement of call() gives."""
    B, L, D, nb = 5, 3, 4, 7
    rng = np.random.default_rng(1)
    for emb in (False, True):
        for nh in (1, 3):
            layer = _layers()[kind](nb, D if emb else -1, num_hash=nh)
            tables = None
            if emb:
                tables = rng.normal(size=(nb * nh, D)) if kind == 'fast' else [rng.normal(size=(nb, D)) for _ in range(nh)]
            for shape in ((B,), (B, L)):
                ids = rng.integers(0, 1000, shape)
                for combiner in ('concat', 'sum', 'mean', None, 'other'):
                    want = O.layer_call(kind, ids, nb, nh, 1, tables, combiner)
                    want = [tuple(w.shape) for w in want] if isinstance(want, list) else tuple(want.shape)
                    assert layer.compute_output_shape(shape, combiner) == want, (emb, nh, shape, combiner)

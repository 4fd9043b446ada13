"""Exact-integer / fp64 oracle of MultiHashLayer and FastMultiHashLayer, written from the published algorithms and independently of
the C code (csrc/hash64.hpp): it works on byte strings, byte by byte -- pure Python integers for single strings, numpy uint64 over groups
of equal-length strings for arrays.

  keras Hashing(num_bins, salt=None)    = FarmHash Fingerprint64(bytes) % num_bins         (unsigned 64-bit)
  keras Hashing(num_bins, salt=(s, s))  = SipHash-2-4 with key (k0, k1) = (s, s) % num_bins
  an integer id is hashed as its decimal text, str(int(id))
"""
import numpy as np

M64 = (1 << 64) - 1
K0, K1, K2 = 0xc3a5c85c97cb3127, 0xb492b66fbe98f273, 0x9ae16a3b2f90404f
MAX_FP_LEN = 32


# ---- one byte string, Python integers ----------------------------------------------------------------------------------------------
def _rotl(v, s):
    return ((v << s) | (v >> (64 - s))) & M64


def _rotr(v, s):
    return ((v >> s) | (v << (64 - s))) & M64


def siphash24(k0, k1, data):
    v0, v1, v2, v3 = k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573

    def rounds(n, v0, v1, v2, v3):
        for _ in range(n):
            v0 = (v0 + v1) & M64; v1 = _rotl(v1, 13); v1 ^= v0; v0 = _rotl(v0, 32)
            v2 = (v2 + v3) & M64; v3 = _rotl(v3, 16); v3 ^= v2
            v0 = (v0 + v3) & M64; v3 = _rotl(v3, 21); v3 ^= v0
            v2 = (v2 + v1) & M64; v1 = _rotl(v1, 17); v1 ^= v2; v2 = _rotl(v2, 32)
        return v0, v1, v2, v3

    n = len(data)
    blocks = [int.from_bytes(data[i:i + 8], 'little') for i in range(0, n - n % 8, 8)]
    blocks.append(int.from_bytes(data[n - n % 8:], 'little') | ((n & 0xff) << 56))
    for m in blocks:
        v3 ^= m
        v0, v1, v2, v3 = rounds(2, v0, v1, v2, v3)
        v0 ^= m
    v2 ^= 0xff
    v0, v1, v2, v3 = rounds(4, v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def _len16(u, v, mul):
    a = ((u ^ v) * mul) & M64
    a ^= a >> 47
    b = ((v ^ a) * mul) & M64
    b ^= b >> 47
    return (b * mul) & M64


def fingerprint64(data):
    """farmhashna::Hash64 for 0..32 bytes (the branches for longer inputs are not implemented)."""
    n = len(data)
    f64 = lambda o: int.from_bytes(data[o:o + 8], 'little')        # noqa: E731
    f32 = lambda o: int.from_bytes(data[o:o + 4], 'little')        # noqa: E731
    mul = (K2 + 2 * n) & M64
    if n > MAX_FP_LEN:
        raise NotImplementedError('Fingerprint64 of %d bytes' % n)
    if n > 16:
        a, b = (f64(0) * K1) & M64, f64(8)
        c, d = (f64(n - 8) * mul) & M64, (f64(n - 16) * K2) & M64
        return _len16((_rotr((a + b) & M64, 43) + _rotr(c, 30) + d) & M64, (a + _rotr((b + K2) & M64, 18) + c) & M64, mul)
    if n >= 8:
        a, b = (f64(0) + K2) & M64, f64(n - 8)
        c = (_rotr(b, 37) * mul + a) & M64
        d = ((_rotr(a, 25) + b) * mul) & M64
        return _len16(c, d, mul)
    if n >= 4:
        return _len16((n + (f32(0) << 3)) & M64, f32(n - 4), mul)
    if n > 0:
        a, b, c = data[0], data[n >> 1], data[n - 1]
        y, z = (a + (b << 8)) & 0xffffffff, (n + (c << 2)) & 0xffffffff
        m = ((y * K2) & M64) ^ ((z * K0) & M64)
        return ((m ^ (m >> 47)) * K2) & M64
    return K2


def bucket(data, salt, num_bins):
    """salt None: the unsalted hash; else SipHash keyed (salt, salt)."""
    h = fingerprint64(data) if salt is None else siphash24(salt, salt, data)
    return h % num_bins


# ---- arrays of equal-length strings, numpy uint64 (wrap-around arithmetic) ----------------------------------------------------------
def _u(v):
    return np.uint64(v)


def _vrotl(v, s):
    return (v << _u(s)) | (v >> _u(64 - s))


def _vrotr(v, s):
    return (v >> _u(s)) | (v << _u(64 - s))


def _vfetch(mat, off, nbytes):
    out = np.zeros(mat.shape[0], dtype=np.uint64)
    for i in range(nbytes):
        if off + i < mat.shape[1]:
            out |= mat[:, off + i].astype(np.uint64) << _u(8 * i)
    return out


def _vsip(k, mat):
    m_rows, n = mat.shape
    k = _u(k)
    v0 = np.full(m_rows, k ^ _u(0x736f6d6570736575), dtype=np.uint64)
    v1 = np.full(m_rows, k ^ _u(0x646f72616e646f6d), dtype=np.uint64)
    v2 = np.full(m_rows, k ^ _u(0x6c7967656e657261), dtype=np.uint64)
    v3 = np.full(m_rows, k ^ _u(0x7465646279746573), dtype=np.uint64)

    def rounds(c, v0, v1, v2, v3):
        for _ in range(c):
            v0 = v0 + v1; v1 = _vrotl(v1, 13); v1 = v1 ^ v0; v0 = _vrotl(v0, 32)
            v2 = v2 + v3; v3 = _vrotl(v3, 16); v3 = v3 ^ v2
            v0 = v0 + v3; v3 = _vrotl(v3, 21); v3 = v3 ^ v0
            v2 = v2 + v1; v1 = _vrotl(v1, 17); v1 = v1 ^ v2; v2 = _vrotl(v2, 32)
        return v0, v1, v2, v3

    blocks = [_vfetch(mat, o, 8) for o in range(0, n - n % 8, 8)]
    blocks.append(_vfetch(mat, n - n % 8, n % 8) | _u((n & 0xff) << 56))
    for m in blocks:
        v3 = v3 ^ m
        v0, v1, v2, v3 = rounds(2, v0, v1, v2, v3)
        v0 = v0 ^ m
    v2 = v2 ^ _u(0xff)
    v0, v1, v2, v3 = rounds(4, v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def _vlen16(u, v, mul):
    a = (u ^ v) * mul
    a = a ^ (a >> _u(47))
    b = (v ^ a) * mul
    b = b ^ (b >> _u(47))
    return b * mul


def _vfp(mat):
    m_rows, n = mat.shape
    if n > MAX_FP_LEN:
        raise NotImplementedError('Fingerprint64 of %d bytes' % n)
    mul = _u((K2 + 2 * n) & M64)
    k0, k1, k2 = _u(K0), _u(K1), _u(K2)
    if n > 16:
        a, b = _vfetch(mat, 0, 8) * k1, _vfetch(mat, 8, 8)
        c, d = _vfetch(mat, n - 8, 8) * mul, _vfetch(mat, n - 16, 8) * k2
        return _vlen16(_vrotr(a + b, 43) + _vrotr(c, 30) + d, a + _vrotr(b + k2, 18) + c, mul)
    if n >= 8:
        a, b = _vfetch(mat, 0, 8) + k2, _vfetch(mat, n - 8, 8)
        return _vlen16(_vrotr(b, 37) * mul + a, (_vrotr(a, 25) + b) * mul, mul)
    if n >= 4:
        return _vlen16(_u(n) + (_vfetch(mat, 0, 4) << _u(3)), _vfetch(mat, n - 4, 4), mul)
    if n > 0:
        a, b, c = (mat[:, i].astype(np.uint64) for i in (0, n >> 1, n - 1))
        y, z = (a + (b << _u(8))) & _u(0xffffffff), (_u(n) + (c << _u(2))) & _u(0xffffffff)
        m = (y * k2) ^ (z * k0)
        return (m ^ (m >> _u(47))) * k2
    return np.full(m_rows, k2, dtype=np.uint64)


def expand_salts(salts, num_hash):
    """The constructor's rule: an int s -> [s, s + 1, ...]; a short list is extended by last + 1."""
    out = [salts + i for i in range(num_hash)] if isinstance(salts, int) else list(salts)
    while len(out) < num_hash:
        out.append(out[-1] + 1)
    return out


def texts_of(values):
    """Flat list of byte strings of an array-like of ints, str or bytes (ints as their decimal text)."""
    flat = np.asarray(values, dtype=object).reshape(-1) if not isinstance(values, np.ndarray) else values.reshape(-1)
    out = []
    for v in flat.tolist():
        if isinstance(v, bytes):
            out.append(v)
        elif isinstance(v, str):
            out.append(v.encode('utf-8'))
        else:
            out.append(str(int(v)).encode('ascii'))
    return out


def buckets(values, num_bins, num_hash, salts, first_unsalted):
    """(n, num_hash) int64 bucket numbers of the flattened `values`."""
    with np.errstate(over='ignore'):
        texts = texts_of(values)
        salts = expand_salts(salts, num_hash)
        out = np.zeros((len(texts), num_hash), dtype=np.int64)
        by_len = {}
        for i, t in enumerate(texts):
            by_len.setdefault(len(t), []).append(i)
        for n, idx in by_len.items():
            mat = np.frombuffer(b''.join(texts[i] for i in idx), dtype=np.uint8).reshape(len(idx), n) if n else np.zeros((len(idx), 0), np.uint8)
            for h in range(num_hash):
                hv = _vfp(mat) if (first_unsalted and h == 0) else _vsip(salts[h], mat)
                out[idx, h] = (hv % _u(num_bins)).astype(np.int64)
        return out


# ---- the layers, fp64 -------------------------------------------------------------------------------------------------------------
def layer_call(kind, values, num_bins, num_hash, salts, tables, combiner):
    """The reference's call().  kind 'multi' | 'fast'; values: array-like of shape (B,) or (B, L); tables: None (no embedding), for 'multi' a
    list of num_hash (num_bins, D) arrays, for 'fast' one (num_bins * num_hash, D) array.  Returns an array or (multi, no matching combiner) a list."""
    shape = np.asarray(values, dtype=object).shape if not isinstance(values, np.ndarray) else values.shape
    bk = buckets(values, num_bins, num_hash, salts, kind == 'fast').reshape(tuple(shape) + (num_hash,))
    emb = tables is not None
    if kind == 'multi':
        outs = [np.asarray(tables[h], dtype=np.float64)[bk[..., h]] if emb else bk[..., h] for h in range(num_hash)]
        if num_hash == 1:
            return outs[0]
        if combiner == 'concat':
            return np.concatenate(outs, axis=-1)
        if combiner == 'sum' and emb:
            return sum(outs[1:], outs[0])
        if combiner == 'mean' and emb:
            return sum(outs[1:], outs[0]) * (1.0 / num_hash)
        return outs
    if emb:
        out = np.asarray(tables, dtype=np.float64)[bk + np.arange(num_hash, dtype=np.int64) * num_bins]      # (..., num_hash, D)
    else:
        out = np.concatenate([bk[..., h] for h in range(num_hash)], axis=-1)
    if combiner == 'concat':
        rest = int(np.prod(out.shape[1:])) if out.ndim > 1 else 1
        return out.reshape(-1, rest)
    if combiner == 'sum' and emb:
        return out.sum(axis=-2)
    if combiner == 'mean' and emb:
        return out.mean(axis=-2)
    return out


def layer_get_pooling(kind, values, num_bins, num_hash, salts, tables, weights=None):
    e = layer_call(kind, values, num_bins, num_hash, salts, tables, 'sum')
    if weights is not None:
        e = np.asarray(weights, dtype=np.float64)[..., None] * e
    if e.ndim > 2:
        return e.sum(axis=tuple(range(1, e.ndim - 1)))
    return e

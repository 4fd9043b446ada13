"""Plain-Python oracle of CartesianProductLayer, independent of rec_now_amd: texts are composed with str() and bytes.join, the invalid patterns
are the reference's regular expressions (built the way rec_now/layers/cartesian_product_layer.py builds them) applied with `re`, and texts are
hashed through _hash_oracle."""
import itertools
import re

import numpy as np

import _hash_oracle as O


def _b(v):
    if isinstance(v, bytes):
        return v
    if isinstance(v, str):
        return v.encode('utf-8')
    return str(int(v)).encode('ascii')


def rows_of(x):
    """The reference's reshape of one input: -> (list of rows of bytes, batch1)."""
    arr = x if isinstance(x, np.ndarray) else np.asarray(x, dtype=object)
    if arr.ndim == 0 or arr.shape[0] == 1:
        return [[_b(v) for v in arr.reshape(-1).tolist()]], True
    flat = arr.reshape(arr.shape[0], -1)
    return [[_b(v) for v in row] for row in flat.tolist()], False


def patterns_of(invalid_pattern_list, separator):
    out = []
    for i, s in enumerate(invalid_pattern_list or []):
        if s is None:
            continue
        parts = ['.*'] * len(invalid_pattern_list)
        parts[i] = '(' + s + ')'
        out.append(re.compile(('^' + separator.join(parts) + '$').encode('utf-8')))
    return out


def texts(inputs, separator='-', invalid_pattern_list=None, default=''):
    """(B, P) object array of bytes."""
    rows = [rows_of(x) for x in inputs]
    sizes = [len(r) for r, b1 in rows if not b1]
    B = sizes[0] if sizes else 1
    regs = patterns_of(invalid_pattern_list, separator)
    sep, dflt = separator.encode('utf-8'), default.encode('utf-8')
    dims = [len(r[0]) for r, _ in rows]
    out = np.empty((B, int(np.prod(dims, dtype=np.int64))), dtype=object)
    for b in range(B):
        fields = [r[0 if b1 else b] for r, b1 in rows]
        for j, idx in enumerate(itertools.product(*[range(n) for n in dims])):
            t = sep.join(f[i] for f, i in zip(fields, idx))
            for rg in regs:
                t = rg.sub(lambda m: dflt, t, count=1)
            out[b, j] = t
    return out


def buckets(text_array, num_bins, num_hash, salts, first_unsalted):
    """(B, P, num_hash) int64."""
    return O.buckets(text_array, num_bins, num_hash, salts, first_unsalted).reshape(tuple(text_array.shape) + (num_hash,))

"""CartesianProductLayer -- drop-in for rec_now/layers/cartesian_product_layer.py: crossed features such as `user_city x item_category`.

The reference casts every input to strings, joins one element of each input as "a-b-c" and returns the (B, L1 * L2 * ... * Ln) string tensor,
which then goes into MultiHashLayer / FastMultiHashLayer.  A GPU has no strings, and the strings are not wanted for themselves, so here

  * integer CUDA tensors give a lazy `CrossedIds`: it holds the input tensors, the separator and the invalid patterns, and launches nothing.
    Handed to a hash layer, ONE kernel (csrc/cross_hash.hip) reads the B x (L1 + ... + Ln) input ids, composes the text of every crossed
    element on chip, hashes it, gathers the rows and reduces; the text of a crossed id never exists in memory.  `.text_bytes()` / `.numpy()`
    materialise the texts for whoever does want them.
  * lists / numpy arrays of str, bytes or ints (also mixed with integer tensors, which are moved to the host) take the host route: plain numpy and
    Python `re`, no GPU call, the (B, P) object array of bytes that TensorFlow's result converts to.  This mirrors how MultiHashLayer treats strings.

Symbols: B batch size; input i is (B,) (Li = 1), (B, Li), (B, Li1, ..., Lik) (Li their product), or a 0-d tensor / a tensor with first dimension 1,
which is ONE row shared by the whole batch; P = L1 * ... * Ln elements per output row, row-major with the last input fastest.

Invalid patterns.  For input i with pattern s the reference replaces the joined text by `default_result_str` when `^.*SEP.*SEP(s)SEP.*$` (the group
in position i) matches it.  The host route applies exactly that with `re`.  The GPU route takes patterns that are alternations of literals ("A1a|na",
"|na", ""), at most 8 alternatives of at most 24 bytes, and decides the SAME regular expression on the joined text -- not a comparison per field: with
the default separator '-' the fields 5 and -1 join to "5--1", which matches `^.*-(1)$` although the second field is not "1".
"""
import itertools
import re

import numpy as np
import torch

from .. import _lib
from ._keras import Layer

_KEY_I32, _KEY_I64 = 2, 3                                        # RECNOW_KEY_I32 / _I64
MAX_INPUTS, MAX_SEP_BYTES, MAX_TEXT_BYTES, MAX_ALTERNATIVES, MAX_LITERAL_BYTES = 4, 4, 96, 8, 24      # RECNOW_CROSS_* of include/recnow.h
_TEXT_BYTES = {torch.int32: 11, torch.int64: 20}                 # the longest decimal text: "-2147483648", "-9223372036854775808"
_META = set('\\.^$*+?()[]{}')                                    # '|' separates the alternatives


def _bytes(s):
    return s if isinstance(s, bytes) else str(s).encode('utf-8')


def gen_invalid_patterns(invalid_pattern_list, separator):
    """The reference's expressions: `^.*SEP(s)SEP.*$` with the group in the position of each pattern that is not None."""
    if invalid_pattern_list is None:
        return []
    out = []
    for i, s in enumerate(invalid_pattern_list):
        if s is None:
            continue
        parts = ['.*'] * len(invalid_pattern_list)
        parts[i] = '(%s)' % s
        out.append('^' + separator.join(parts) + '$')
    return out


def _check_ids_dtype(t):
    if t.dtype.is_floating_point or t.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise TypeError('CartesianProductLayer crosses ids: integer tensors (int32 / int64) or strings, got a %s tensor' % t.dtype)


def _as_rows(shape):
    """The reference's reshape: -> (rows, L, batch1)."""
    shape = tuple(int(v) for v in shape)
    n = 1
    for v in shape:
        n *= v
    if len(shape) == 0 or shape[0] == 1:
        return 1, n, True
    return shape[0], (n // shape[0] if shape[0] else int(np.prod(shape[1:], dtype=np.int64))), False


def _batch_size(rows):
    """rows: [(rows_i, batch1_i)] -> B (1 when every input is one shared row)."""
    sizes = sorted(set(r for r, b1 in rows if not b1))
    if len(sizes) > 1:
        raise ValueError('inputs disagree on the batch size: %s' % sizes)
    return sizes[0] if sizes else 1


class CrossedIds(object):
    """The (B, P) cross of integer id tensors, not materialised.  MultiHashLayer / FastMultiHashLayer take it wherever they take ids."""

    def __init__(self, inputs, separator='-', invalid_pattern_list=None, default_result_str=''):
        if len(inputs) < 1 or len(inputs) > MAX_INPUTS:
            raise NotImplementedError('a cross of %d inputs: the kernels take at most %d inputs' % (len(inputs), MAX_INPUTS))
        if invalid_pattern_list is not None and len(invalid_pattern_list) != len(inputs):
            raise ValueError('length not equal:%s v.s %s' % (len(invalid_pattern_list), len(inputs)))
        self.separator = _bytes(separator)
        if len(self.separator) > MAX_SEP_BYTES:
            raise NotImplementedError('separator %r: the kernels take a separator of at most %d bytes' % (separator, MAX_SEP_BYTES))
        self.inputs, self.batch1, rows = [], [], []
        for t in inputs:
            _check_ids_dtype(t)
            r, L, b1 = _as_rows(t.shape)
            t = t if t.dtype == torch.int64 else t.to(torch.int32)
            self.inputs.append(t.reshape(r, L).contiguous())
            self.batch1.append(b1)
            rows.append((r, b1))
        B = _batch_size(rows)
        P = 1
        for t in self.inputs:
            P *= int(t.shape[1])
        self.shape = (B, P)
        self.device = self.inputs[0].device
        self.worst_text_bytes = sum(_TEXT_BYTES[t.dtype] for t in self.inputs) + (len(inputs) - 1) * len(self.separator)
        if self.worst_text_bytes > MAX_TEXT_BYTES:
            raise NotImplementedError('the longest text of this cross has %d bytes (11 per int32 input, 20 per int64 input, plus the separators); '
                                      'the kernels compose at most %d bytes' % (self.worst_text_bytes, MAX_TEXT_BYTES))
        self.default = _bytes(default_result_str)
        if len(self.default) > MAX_TEXT_BYTES:
            raise NotImplementedError('default_result_str of %d bytes: the kernels take at most %d bytes' % (len(self.default), MAX_TEXT_BYTES))
        self.spec = self._compile(invalid_pattern_list, separator)

    @staticmethod
    def _compile(patterns, separator):
        """-> per input None or the tuple of literal alternatives (bytes)."""
        if patterns is None or all(s is None for s in patterns):
            return None
        host = 'pass lists / numpy arrays (the host route of CartesianProductLayer takes full regular expressions)'
        sep = separator.decode('utf-8') if isinstance(separator, bytes) else str(separator)
        if _META & set(sep) or '|' in sep or '\n' in sep:
            raise NotImplementedError('separator %r reads as a regular expression inside the invalid patterns; the GPU route takes literal separators: %s'
                                      % (sep, host))
        spec = []
        for s in patterns:
            if s is None:
                spec.append(None)
                continue
            s = s.decode('utf-8') if isinstance(s, bytes) else str(s)
            if _META & set(s) or '\n' in s:
                raise NotImplementedError('invalid pattern %r: the GPU route takes alternations of literals ("a|b"); %s' % (s, host))
            alts = tuple(a.encode('utf-8') for a in s.split('|'))
            if len(alts) > MAX_ALTERNATIVES:
                raise NotImplementedError('invalid pattern %r has %d alternatives: the GPU route takes at most %d alternatives; %s'
                                          % (s, len(alts), MAX_ALTERNATIVES, host))
            for a in alts:
                if len(a) > MAX_LITERAL_BYTES:
                    raise NotImplementedError('literal %r of an invalid pattern has %d bytes: the GPU route takes at most %d bytes; %s'
                                              % (a, len(a), MAX_LITERAL_BYTES, host))
            spec.append(alts)
        return tuple(spec)

    @property
    def has_patterns(self):
        return self.spec is not None and any(s is not None for s in self.spec)

    @property
    def longest_bytes(self):
        """What a hash function must take: the worst-case text, and the default string where a pattern can put it in."""
        return max(self.worst_text_bytes, len(self.default) if self.has_patterns else 0)

    def desc(self, default_buckets=None):
        """recnow_cross_desc for the current input tensors (they stay referenced by self)."""
        d = _lib.CrossDesc()
        for k, t in enumerate(self.inputs):
            d.ids[k] = t.data_ptr()
            d.dtype[k] = _KEY_I64 if t.dtype == torch.int64 else _KEY_I32
            d.len[k] = int(t.shape[1])
            d.batch1[k] = 1 if self.batch1[k] else 0
        d.n_inputs = len(self.inputs)
        d.sep_len = len(self.separator)
        d.sep_word = int.from_bytes(self.separator, 'little')
        d.default_len = len(self.default)
        if self.has_patterns:
            for k, alts in enumerate(self.spec):
                if alts is None:
                    continue
                d.n_alt[k] = len(alts)
                for a, lit in enumerate(alts):
                    d.lit_len[k][a] = len(lit)
                    for q in range(3):
                        d.lit_words[k][a][q] = int.from_bytes(lit[8 * q:8 * q + 8], 'little')
            for q in range(MAX_TEXT_BYTES // 8):
                d.default_words[q] = int.from_bytes(self.default[8 * q:8 * q + 8], 'little')
            if default_buckets is not None:
                for h, v in enumerate(default_buckets):
                    d.default_buckets[h] = int(v)
        return d

    def text_bytes(self):
        """On the GPU: (B, P, W) uint8 texts, zero padded, and (B, P) int32 lengths; W the longest possible text rounded up to 8."""
        _lib.require_gpu(self.inputs[0], 'CartesianProductLayer input')
        B, P = self.shape
        W = max(8, -(-self.longest_bytes // 8) * 8)
        text = torch.empty((B, P, W), dtype=torch.uint8, device=self.device)
        lens = torch.empty((B, P), dtype=torch.int32, device=self.device)
        _lib.call('recnow_cross_text', self.desc(), B, W, _lib.ptr(text), _lib.ptr(lens), _lib.stream())
        return text, lens

    def numpy(self):
        """(B, P) numpy object array of bytes -- what the reference's string tensor converts to."""
        text, lens = self.text_bytes()
        text, lens = text.cpu().numpy(), lens.cpu().numpy()
        B, P = self.shape
        out = np.empty((B, P), dtype=object)
        for b in range(B):
            for j in range(P):
                out[b, j] = text[b, j, :lens[b, j]].tobytes()
        return out


def _host_rows(x):
    """One input of the host route -> (rows, L) object array of bytes, batch1."""
    if isinstance(x, torch.Tensor):
        _check_ids_dtype(x)
        x = x.detach().cpu().numpy()
    arr = x if isinstance(x, np.ndarray) else np.asarray(x, dtype=object)
    if arr.dtype.kind in 'fcb':
        raise TypeError('CartesianProductLayer crosses ids: integers or strings, got a %s array' % arr.dtype)
    r, L, b1 = _as_rows(arr.shape)
    out = np.empty((r, L), dtype=object)
    for i, v in enumerate(arr.reshape(-1).tolist()):
        if isinstance(v, (bytes, str)):
            v = _bytes(v)
        elif isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            v = str(int(v)).encode('ascii')
        else:
            raise TypeError('CartesianProductLayer crosses ids: integers or strings, got %s' % type(v).__name__)
        out[i // L if L else 0, i % L if L else 0] = v
    return out, b1


def cross_on_host(inputs, separator='-', invalid_pattern_list=None, default_result_str=''):
    """The reference's call() in numpy and `re`: (B, P) object array of bytes."""
    if invalid_pattern_list is not None and len(invalid_pattern_list) != len(inputs):
        raise ValueError('length not equal:%s v.s %s' % (len(invalid_pattern_list), len(inputs)))
    rows = [_host_rows(x) for x in inputs]
    B = _batch_size([(a.shape[0], b1) for a, b1 in rows])
    sep, default = _bytes(separator), _bytes(default_result_str)
    sep_text = sep.decode('utf-8') if isinstance(separator, bytes) else str(separator)
    regs = [re.compile(p.encode('utf-8')) for p in gen_invalid_patterns(
        None if invalid_pattern_list is None else [None if s is None else (s.decode('utf-8') if isinstance(s, bytes) else str(s))
                                                   for s in invalid_pattern_list], sep_text)]
    dims = [a.shape[1] for a, _ in rows]
    P = int(np.prod(dims, dtype=np.int64))
    out = np.empty((B, P), dtype=object)
    for b in range(B):
        fields = [a[0 if b1 else b] for a, b1 in rows]
        for j, idx in enumerate(itertools.product(*[range(n) for n in dims])):
            text = sep.join(f[i] for f, i in zip(fields, idx))
            for rg in regs:
                text = rg.sub(lambda m: default, text, count=1)
            out[b, j] = text
    return out


class CartesianProductLayer(Layer):
    """Cartesian product of the inputs' elements, each cast to its text and joined by `separator` (see the module docstring)."""

    def __init__(self, separator='-', trainable=True, name=None, dtype=None, dynamic=False, **kwargs):
        super().__init__(trainable=trainable, name=name, dtype=dtype, dynamic=dynamic, **kwargs)
        self.separator = separator

    def build(self, input_shape=None):
        self.built = True

    def forward(self, inputs, *args, **kwargs):
        if not self.built:
            self.build(None)
        return self.call(inputs, *args, **kwargs)

    def call(self, inputs, invalid_pattern_list=None, default_result_str=""):
        """inputs: list of 1..4 tensors / arrays.  invalid_pattern_list: None, or one pattern (or None) per input: an element whose joined text
        matches `^.*SEP(pattern)SEP.*$`, the group in that input's position, becomes default_result_str.
        Returns a CrossedIds (every input an integer CUDA tensor) or a (B, P) numpy object array of bytes (host route)."""
        if not isinstance(inputs, (list, tuple)):
            raise TypeError('CartesianProductLayer takes a list of inputs, got %s' % type(inputs).__name__)
        for x in inputs:
            if isinstance(x, torch.Tensor):
                _check_ids_dtype(x)
        if len(inputs) > 0 and all(isinstance(x, torch.Tensor) and x.is_cuda for x in inputs):
            return CrossedIds(inputs, self.separator, invalid_pattern_list, default_result_str)
        return cross_on_host(inputs, self.separator, invalid_pattern_list, default_result_str)

"""MultiHashLayer / FastMultiHashLayer -- drop-ins for rec_now/layers/multi_hash_layer.py: the step that turns a raw id into an embedding.

An id is hashed by `num_hash` differently salted hash functions into `num_bins` buckets, each bucket selects a row of an embedding table
and the rows are combined (the multi-hash trick: a small table stands in for a huge vocabulary).  The reference hashes on the host --
integer ids go through `tf.strings.as_string` first -- and looks the buckets up afterwards.  Here integer ids stay on the GPU: one HIP kernel
(csrc/hash_embed.hip) formats, hashes, gathers and reduces in one pass, so no (B, L, num_hash) index tensor and no (B, L, num_hash, D) or
(B, L, D) temporary exists; `get_pooling` is one launch down to (B, D).  The table gradient goes through the sorted-segment reduction of
csrc/embed.hip (bit-identical from run to run).  A `CrossedIds` (CartesianProductLayer on integer tensors) is taken wherever ids are: the kernels of
csrc/cross_hash.hip compose the "a-b" text of every crossed element on chip and hash it in the same launch.

Hash functions (csrc/hash64.hpp, one source for host and device): keras `Hashing(num_bins, salt=(s, s))` is SipHash-2-4 keyed (s, s), `% num_bins`;
`Hashing(num_bins, salt=None)` is FarmHash Fingerprint64, `% num_bins` (unsigned 64-bit).  An integer is hashed as its decimal text.  Buckets of
texts of up to 16 bytes are pinned by the reference's own goldens; the 17..32-byte branch of Fingerprint64 (integer ids at or above 10^16, most
negative ids of 17+ digits, under the unsalted first hash of FastMultiHashLayer) is implemented from the published algorithm and agrees between
device, host and an independent oracle, but is NOT yet confirmed against TensorFlow.  Longer texts under the unsalted hash: NotImplementedError.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..rec_block._segments import build_segments
from ._keras import Layer, get_initializer
from .cartesian_product_layer import CrossedIds

_KEY_I32, _KEY_I64, _BUCKETS = 2, 3, 4                           # RECNOW_KEY_I32 / _I64, RECNOW_HASH_BUCKETS
_CROSS = 5                                                       # host side only: the ids are a CrossedIds (csrc/cross_hash.hip)
MODE_SUM, MODE_MEAN, MODE_ROWS, MODE_POOLED = 0, 1, 2, 3         # RECNOW_HASH_*
MAX_NUM_HASH = 16                                                # RN_HASH_MAX_NUM_HASH of csrc/hash64.hpp
MAX_UNSALTED_BYTES = 32                                          # RN_HASH_MAX_FP_LEN


def _default_initializer(shape, generator=None):
    """keras RandomUniform(-1e-4, 1e-4), the reference's default."""
    return (torch.rand(tuple(shape), generator=generator) * 2.0 - 1.0) * 1e-4


def expand_salts(salts, num_hash):
    """An int s -> [s, s + 1, ...]; a list shorter than num_hash is extended by last + 1."""
    out = [salts + i for i in range(num_hash)] if isinstance(salts, int) else list(salts)
    while len(out) < num_hash:
        out.append(out[-1] + 1)
    return out


def _i64_array(values):
    return (ctypes.c_int64 * len(values))(*values)


def hash_strings_host(values, num_bins, salts, first_unsalted):
    """(n, num_hash) int64 numpy bucket numbers of a flat list of str / bytes, hashed on the host by the library (no GPU call)."""
    texts = [v if isinstance(v, bytes) else str(v).encode('utf-8') for v in values]
    if first_unsalted:
        for t in texts:
            if len(t) > MAX_UNSALTED_BYTES:
                raise NotImplementedError('the unsalted hash (Fingerprint64) is implemented for texts of up to %d bytes, got one of %d bytes'
                                          % (MAX_UNSALTED_BYTES, len(t)))
    n, nh = len(texts), len(salts)
    out = np.zeros((n, nh), dtype=np.int64)
    if n == 0:
        return out
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offsets[1:])
    buf = np.frombuffer(b''.join(texts) + b'\0', dtype=np.uint8).copy()
    _lib.call('recnow_hash_bytes_host', buf.ctypes.data, offsets.ctypes.data, n, ctypes.cast(_i64_array(salts), ctypes.c_void_p), nh,
              1 if first_unsalted else 0, int(num_bins), out.ctypes.data)
    return out


class _HashEmbedFunction(torch.autograd.Function):
    """Hash + gather + reduce as one node.  Saves the bucket keys only (and the pooled mode's weights)."""

    @staticmethod
    def forward(ctx, meta, ids, weights, *tables):
        id_dtype, shape, B, L, salts, first_unsalted, num_bins, D, mode, one_table = meta
        nh = len(salts)
        tabs = [_lib.f32c(t.detach(), 'embedding table') for t in tables]
        dev = tabs[0].device
        step = num_bins * D * 4
        bases = [tabs[0].data_ptr() + h * step for h in range(nh)] if one_table else [t.data_ptr() for t in tabs]
        tab_arr = (ctypes.c_void_p * nh)(*bases)
        need_dt = any(ctx.needs_input_grad[3:])
        need_dw = weights is not None and ctx.needs_input_grad[2]
        n = B * L
        keys = torch.empty((n, nh), dtype=torch.int64, device=dev) if (need_dt or need_dw) else None
        keys32 = torch.empty((n, nh), dtype=torch.int32, device=dev) if need_dt else None
        if mode == MODE_POOLED:
            out_shape = (B, D)
        elif mode == MODE_ROWS:
            out_shape = tuple(shape) + (nh, D)
        else:
            out_shape = tuple(shape) + (D,)
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)        # every element is written by the kernel
        wc = _lib.f32c(weights.detach(), 'weights') if weights is not None else None
        if id_dtype == _CROSS:      # ids: (CrossedIds, the default string's buckets); the kernel composes and hashes the texts itself
            _lib.call('recnow_cross_hash_embed_fwd', ids[0].desc(ids[1]), B, ctypes.cast(_i64_array(salts), ctypes.c_void_p), nh,
                      1 if first_unsalted else 0, num_bins, ctypes.cast(tab_arr, ctypes.c_void_p), D, _lib.ptr(wc), mode, _lib.ptr(out),
                      _lib.ptr(keys), _lib.ptr(keys32), _lib.stream())
        else:
            _lib.call('recnow_hash_embed_fwd', _lib.ptr(ids), id_dtype, B, L, ctypes.cast(_i64_array(salts), ctypes.c_void_p), nh,
                      1 if first_unsalted else 0, num_bins, ctypes.cast(tab_arr, ctypes.c_void_p), D, _lib.ptr(wc), mode, _lib.ptr(out),
                      _lib.ptr(keys), _lib.ptr(keys32), _lib.stream())
        saved = [keys, keys32, wc if need_dt else None] + (tabs if need_dw else [])
        ctx.save_for_backward(*saved)
        ctx.meta = (B, L, nh, num_bins, D, mode, one_table, need_dt, need_dw, len(tables))
        return out

    @staticmethod
    def backward(ctx, dout):
        keys, keys32, wc, *tabs = ctx.saved_tensors
        B, L, nh, num_bins, D, mode, one_table, need_dt, need_dw, n_tables = ctx.meta
        n = B * L
        dweights, dtables = None, [None] * n_tables
        if not (need_dt or need_dw):
            return (None, None, None) + tuple(dtables)
        dout = _lib.f32c(dout, 'grad')
        dev = dout.device
        if need_dw:
            dweights = torch.empty((B, L), dtype=torch.float32, device=dev)
            step = num_bins * D * 4
            bases = [tabs[0].data_ptr() + h * step for h in range(nh)] if one_table else [t.data_ptr() for t in tabs]
            tab_arr = (ctypes.c_void_p * nh)(*bases)
            _lib.call('recnow_hash_embed_bwd_weights', _lib.ptr(keys), ctypes.cast(tab_arr, ctypes.c_void_p), nh, num_bins, D, _lib.ptr(dout),
                      B, L, _lib.ptr(dweights), _lib.stream())
        if need_dt:
            V, N = nh * num_bins, n * nh
            dtable = torch.zeros((V, D), dtype=torch.float32, device=dev)
            if N > 0:
                if mode == MODE_MEAN:
                    dout = dout * (1.0 / nh)
                # entry e = id * num_hash + h takes gradient row e / C: its id's (sum, mean), its own (rows), its batch row's (pooled)
                C = {MODE_SUM: nh, MODE_MEAN: nh, MODE_ROWS: 1, MODE_POOLED: L * nh}[mode]
                s = build_segments(keys32.reshape(-1))
                ws = _lib.workspace(_lib.load().recnow_embed_rows_bwd_workspace_bytes(N, D), dev)
                _lib.call('recnow_embed_rows_bwd_direct', _lib.ptr(keys), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first),
                          _lib.ptr(s.n_seg), _lib.ptr(wc) if mode == MODE_POOLED else None, nh, _lib.ptr(dout), N, C, D, _lib.ptr(dtable), V,
                          _lib.ptr(ws), ws.numel(), _lib.stream())
            if one_table:
                dtables = [dtable]
            else:       # the num_hash gradients are views of the one buffer
                dtables = [g if ctx.needs_input_grad[3 + h] else None for h, g in enumerate(dtable.view(nh, num_bins, D).unbind(0))]
        return (None, None, dweights) + tuple(dtables)


class _HashLayerBase(Layer):
    _FAST = False

    def __init__(self, num_bins, embedding_dim=-1, num_hash=2, salts=1, embeddings_initializer=None, trainable=True, name=None,
                 dtype=None, dynamic=False, **kwargs):
        """num_bins: buckets per hash function; embedding_dim > 0: embed into that many dimensions, <= 0: return the bucket numbers;
        num_hash: number of hash functions; salts: an int s (-> s, s + 1, ...) or a list (extended by last + 1);
        embeddings_initializer: `f(shape) -> tensor` or a name _keras.get_initializer knows; default uniform in [-1e-4, 1e-4]."""
        super().__init__(trainable=trainable, name=name, dtype=dtype, dynamic=dynamic, **kwargs)
        if int(num_bins) < 1:
            raise ValueError('num_bins must be at least 1, got %s' % (num_bins,))
        if int(num_hash) < 1:
            raise ValueError('num_hash must be at least 1, got %s' % (num_hash,))
        if int(num_hash) > MAX_NUM_HASH:
            raise NotImplementedError('num_hash = %s: the kernels take at most %d hash functions' % (num_hash, MAX_NUM_HASH))
        self.num_bins = int(num_bins)
        self.embedding_dim = int(embedding_dim)
        self.num_hash = int(num_hash)
        self.salts = [int(s) for s in expand_salts(salts, self.num_hash)]
        if any(s < 0 for s in self.salts):
            raise ValueError('salts must not be negative (they are unsigned 64-bit hash keys), got %s' % (self.salts,))
        if self.embedding_dim > 0:
            if self.num_bins * self.num_hash >= (1 << 31):
                raise ValueError('num_bins * num_hash = %d table rows; the kernels address fewer than 2^31' % (self.num_bins * self.num_hash))
            self.embeddings_initializer = _default_initializer if embeddings_initializer is None else get_initializer(embeddings_initializer)

    # -- weights -------------------------------------------------------------------------------------------------------------------
    def build(self, input_shape=None):
        if self.built:
            return
        if self._build_device is None and torch.cuda.is_available():
            self._build_device = torch.device('cuda')                # get() on demand, or string inputs: the tables live on the GPU
        self.tables = []
        if self.embedding_dim > 0:
            if self._FAST:
                self.tables = [self.add_weight(name='embedding_layer/embeddings', shape=[self.num_bins * self.num_hash, self.embedding_dim],
                                               initializer=self.embeddings_initializer, trainable=self.trainable)]
            else:
                self.tables = [self.add_weight(name='embedding_layers/%d/embeddings' % i, shape=[self.num_bins, self.embedding_dim],
                                               initializer=self.embeddings_initializer, trainable=self.trainable)
                               for i in range(self.num_hash)]
        self.built = True

    # -- shapes (host only) ----------------------------------------------------------------------------------------------------------
    def compute_output_shape(self, input_shape, combiner='sum'):
        """Shape of call(inputs, combiner) for inputs of `input_shape` ((B,) or (B, L)); a list of shapes where call returns a list."""
        s, nh, D = tuple(int(v) for v in input_shape), self.num_hash, self.embedding_dim
        emb = D > 0
        rest = 1
        for v in s[1:]:
            rest *= v
        if not self._FAST:
            one = s + (D,) if emb else s
            if nh == 1:
                return one
            if combiner == 'concat':
                return one[:-1] + (one[-1] * nh,)
            if combiner in ('sum', 'mean') and emb:
                return one
            return [one] * nh
        out = s + (nh, D) if emb else s[:-1] + (s[-1] * nh,)
        if combiner == 'concat':
            r = 1
            for v in out[1:]:
                r *= v
            total = r * out[0]
            return (total // r if r else 0, r)
        if combiner in ('sum', 'mean') and emb:
            return s + (D,)
        return out

    # -- inputs ----------------------------------------------------------------------------------------------------------------------
    def _plan_inputs(self, inputs):
        """-> (ids tensor or numpy buckets, id_dtype, shape).  Integer GPU tensors are hashed by the kernels; str / bytes arrays on the host;
        a CrossedIds (CartesianProductLayer) -> ((it, its default string's buckets), _CROSS, its (B, P))."""
        if isinstance(inputs, CrossedIds):
            return self._plan_cross(inputs), _CROSS, tuple(inputs.shape)
        if isinstance(inputs, torch.Tensor):
            if inputs.dtype.is_floating_point or inputs.dtype in (torch.bool, torch.complex64, torch.complex128):
                raise TypeError('%s hashes integer ids (int32 / int64) or strings, got a %s tensor' % (type(self).__name__, inputs.dtype))
            _lib.require_gpu(inputs, '%s input' % type(self).__name__)
            if inputs.dim() < 1:
                raise ValueError('inputs must have a batch axis: (B,) or (B, L)')
            if inputs.dtype == torch.int64:
                return inputs.contiguous(), _KEY_I64, tuple(inputs.shape)
            return inputs.to(torch.int32).contiguous(), _KEY_I32, tuple(inputs.shape)
        arr = np.asarray(inputs, dtype=object) if not isinstance(inputs, np.ndarray) else inputs
        flat = arr.reshape(-1).tolist()
        if arr.ndim < 1 or not all(isinstance(v, (str, bytes)) for v in flat):
            raise TypeError('%s takes an int32 / int64 CUDA tensor, or a (nested) list / numpy array of str or bytes; got %s. '
                            'rec_now_amd computes only on the GPU: move integer ids with torch.as_tensor(ids).cuda(); there is no CPU fallback.'
                            % (type(self).__name__, type(inputs).__name__))
        return hash_strings_host(flat, self.num_bins, self.salts, self._FAST), _BUCKETS, tuple(arr.shape)

    def _plan_cross(self, crossed):
        """The limits a cross must keep under this layer, checked before any launch; the buckets of its default string, hashed on the host."""
        longest = max(crossed.worst_text_bytes, len(crossed.default))
        if self._FAST and longest > MAX_UNSALTED_BYTES:
            raise NotImplementedError('%s: the unsalted hash (Fingerprint64) is implemented for texts of up to %d bytes; this cross can reach %d bytes '
                                      '(11 per int32 input, 20 per int64 input, the separators; or the default string). MultiHashLayer takes it.'
                                      % (type(self).__name__, MAX_UNSALTED_BYTES, longest))
        B, P = crossed.shape
        if B * P * self.num_hash >= (1 << 31):
            raise NotImplementedError('B * P * num_hash = %d * %d * %d: the kernels address fewer than 2^31 crossed entries' % (B, P, self.num_hash))
        _lib.require_gpu(crossed.inputs[0], '%s input' % type(self).__name__)
        default_buckets = None
        if crossed.has_patterns:
            default_buckets = hash_strings_host([crossed.default], self.num_bins, self.salts, self._FAST)[0].tolist()
        return crossed, default_buckets

    def _buckets(self, ids, id_dtype, shape):
        """(shape..., num_hash) int64 bucket numbers (embedding_dim <= 0)."""
        nh = self.num_hash
        if id_dtype == _BUCKETS:
            return torch.from_numpy(ids).reshape(tuple(shape) + (nh,))          # hashed on the host already: stays there
        if id_dtype == _CROSS:
            out = torch.empty(tuple(shape) + (nh,), dtype=torch.int64, device=ids[0].device)
            _lib.call('recnow_cross_hash_ids', ids[0].desc(ids[1]), shape[0], ctypes.cast(_i64_array(self.salts), ctypes.c_void_p), nh,
                      1 if self._FAST else 0, self.num_bins, _lib.ptr(out), _lib.stream())
            return out
        out = torch.empty(tuple(shape) + (nh,), dtype=torch.int64, device=ids.device)
        _lib.call('recnow_hash_ids', _lib.ptr(ids), id_dtype, ids.numel(), ctypes.cast(_i64_array(self.salts), ctypes.c_void_p), nh,
                  1 if self._FAST else 0, self.num_bins, _lib.ptr(out), _lib.stream())
        return out

    def _embed(self, ids, id_dtype, shape, mode, weights=None):
        dev = self.tables[0].device
        if id_dtype == _BUCKETS:
            if dev.type != 'cuda':
                _lib.require_gpu(self.tables[0], 'embedding table')
            ids = torch.from_numpy(ids).to(dev)
        n = 1
        for v in shape:
            n *= v
        B = shape[0]
        L = n // B if B else (int(np.prod(shape[1:])) if len(shape) > 1 else 1)
        if mode == MODE_POOLED and weights is not None:
            _lib.require_gpu(weights, 'weights')
            if tuple(weights.shape) != tuple(shape):
                raise ValueError('weights must have the shape of keys, got %s and %s' % (tuple(weights.shape), tuple(shape)))
        if mode == MODE_POOLED and (self.embedding_dim if self.embedding_dim % 4 else self.embedding_dim // 4) > 256:
            raise NotImplementedError('get_pooling: embedding_dim = %d is wider than the fused kernel pools' % self.embedding_dim)
        meta = (id_dtype, tuple(shape), B, L, tuple(self.salts), self._FAST, self.num_bins, self.embedding_dim, mode, self._FAST)
        return _HashEmbedFunction.apply(meta, ids, weights, *self.tables)

    # -- reference API ---------------------------------------------------------------------------------------------------------------
    def forward(self, inputs, *args, **kwargs):
        if not self.built and isinstance(inputs, (torch.Tensor, CrossedIds)):
            self._build_device = inputs.device
        if not self.built:
            self.build(None)
        return self.call(inputs, *args, **kwargs)

    def get(self, inputs):
        if not self.built:
            if isinstance(inputs, (torch.Tensor, CrossedIds)):
                self._build_device = inputs.device
            self.build()
        return self(inputs, combiner='sum')

    def get_pooling(self, keys, weights=None, name=None):
        """sum over every axis between the first and the last of weights[..., None] * get(keys): (B, D).  One fused launch."""
        if self.embedding_dim <= 0:
            raise ValueError('get_pooling needs embedding_dim > 0')
        if not self.built:
            if isinstance(keys, (torch.Tensor, CrossedIds)):
                self._build_device = keys.device
            self.build()
        ids, id_dtype, shape = self._plan_inputs(keys)
        return self._embed(ids, id_dtype, shape, MODE_POOLED, weights)


class MultiHashLayer(_HashLayerBase):
    """num_hash salted hash functions (SipHash keyed (salts[i], salts[i])), one (num_bins, D) table each.

    Symbols: B batch size, L ids per row (inputs are (B,) or (B, L)), D embedding dim, Nh number of hash functions.
    Weights: `embedding_layers/{i}/embeddings` (num_bins, D), i < Nh -- the reference's `embedding_layers[i].embeddings`.
    """
    _FAST = False

    def call(self, inputs, combiner='sum'):
        """combiner 'concat' | 'sum' | 'mean' | anything else (a list of the Nh outputs).  One hash function: its output, whatever the combiner."""
        ids, id_dtype, shape = self._plan_inputs(inputs)
        nh = self.num_hash
        if self.embedding_dim <= 0:
            outs = list(self._buckets(ids, id_dtype, shape).unbind(-1))
            if nh == 1:
                return outs[0]
            if combiner == 'concat':
                return torch.cat(outs, dim=-1)                      # (B, Nh * L), hash-major, as the reference
            return outs
        if nh == 1 or combiner == 'sum':
            return self._embed(ids, id_dtype, shape, MODE_SUM)
        if combiner == 'mean':
            return self._embed(ids, id_dtype, shape, MODE_MEAN)
        rows = self._embed(ids, id_dtype, shape, MODE_ROWS)        # (..., Nh, D)
        if combiner == 'concat':
            return rows.reshape(tuple(shape) + (nh * self.embedding_dim,))
        return list(rows.unbind(-2))


class FastMultiHashLayer(_HashLayerBase):
    """Hash function 0 unsalted (FarmHash Fingerprint64), hash i > 0 SipHash keyed (salts[i], salts[i]); ONE (num_bins * Nh, D) table, hash i
    owning rows i * num_bins .. (i + 1) * num_bins.

    Weights: `embedding_layer/embeddings` (num_bins * Nh, D) -- the reference's `embedding_layer.embeddings`.
    """
    _FAST = True

    def call(self, inputs, combiner='sum'):
        """Without embedding: (B, Nh * L) bucket numbers ('concat': reshaped to (B, -1)).  With: 'concat' (B, L * Nh * D), 'sum' / 'mean'
        (B, L, D), anything else (B, L, Nh, D)."""
        ids, id_dtype, shape = self._plan_inputs(inputs)
        if self.embedding_dim <= 0:
            out = torch.cat(list(self._buckets(ids, id_dtype, shape).unbind(-1)), dim=-1)
        elif combiner == 'sum':
            return self._embed(ids, id_dtype, shape, MODE_SUM)
        elif combiner == 'mean':
            return self._embed(ids, id_dtype, shape, MODE_MEAN)
        else:
            out = self._embed(ids, id_dtype, shape, MODE_ROWS)
        if combiner == 'concat':
            rest = 1
            for v in out.shape[1:]:
                rest *= v
            out = out.reshape(-1, rest)
        return out

"""Pooled embedding lookup by slot -- drop-in for the pooled-lookup path of rec_now/rec_block/embedding_util.py
(/root/reference/rec_now/rec_block/embedding_util.py:138-195 `sparse_batch_segment_ids_of_targets` and :239-324
`embedding_using_sparse_batch_segment_ids`): the step that produces the (B, T, D) field embeddings the interaction layers
consume.  Host side of the HIP kernels in csrc/embed.hip; ids are sorted / uniqued with the same radix-sort machinery as
the in-batch losses (rec_block/_segments.py).

The rest of the reference module is here too (second half of this file): fetch_single_slot, embedding_single_slot and pool_slots on the
kernels of csrc/slot_fetch.hip, and the small helpers (isin, mask_values, first_occurance_in_row, batch_segment_ids_of_targets,
pool_single_slot, the two older pooled lookups) on recnow_slot_targets and a few torch ops.
"""
import warnings

import torch

from .. import _lib
from ._segments import build_segments

_KEY_I32, _KEY_I64 = 2, 3


def _slot_tensor(slots):
    if not isinstance(slots, torch.Tensor):
        slots = torch.as_tensor(slots, device='cuda')
    _lib.require_gpu(slots, 'slots')
    if slots.dtype == torch.int64:
        return slots.contiguous(), _KEY_I64, torch.int64
    if slots.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8):
        return slots.to(torch.int32).contiguous(), _KEY_I32, torch.int32
    raise TypeError('slots must be an integer tensor (string slots of the reference are hashed upstream); got %s' % slots.dtype)


def _slot_targets(slots, target_slots, ids, want_key, id_limit=0):
    """(B,C) slots -> seg (B,C) int32 target index or -1, and optionally the int64 sort key (id, or KEY_NOT_POOLED).
    id_limit = V (a table of V < 2^31 - 1 rows): entries that are not pooled and ids outside the table carry the key V instead, and a
    third value -- the same keys as int32 -- is returned for the sort (one key word: three digit passes for V = 2^20 instead of four)."""
    if not isinstance(target_slots, list):
        target_slots = list(target_slots)
    if len(set(target_slots)) != len(target_slots):
        raise ValueError('target_slots must not contain duplicates')       # the reference's StaticHashTable rejects them too
    slots, sdt, tdt = _slot_tensor(slots)
    if slots.dim() != 2:
        raise ValueError('slots must be a (B, C) matrix')
    dev = slots.device
    targets = _lib.const_array(target_slots, tdt, dev)
    seg = torch.empty(slots.shape, dtype=torch.int32, device=dev)
    key = torch.empty(slots.shape, dtype=torch.int64, device=dev) if want_key else None
    narrow = bool(want_key and 0 < id_limit < (1 << 31) - 1)
    key32 = torch.empty(slots.shape, dtype=torch.int32, device=dev) if narrow else None
    _lib.call('recnow_slot_targets', _lib.ptr(slots), sdt, _lib.ptr(targets), len(target_slots), _lib.ptr(ids) if want_key else None,
              slots.numel(), _lib.ptr(seg), _lib.ptr(key), int(id_limit) if narrow else 0, _lib.ptr(key32), _lib.stream())
    if id_limit:
        return seg, key, key32
    return seg, key


def sparse_batch_segment_ids_of_targets(slots, target_slots):
    """embedding_util.py:138-195.  Returns (mask (B,C) bool, sp_segment_ids (n,) int32 = row * T + target index of the
    masked-in entries in row-major order, num_rows, num_ids, num_segments).  The compaction has a data-dependent size, so
    this (API-parity) function synchronises; the pooled lookup below never materialises it."""
    if not isinstance(target_slots, list):
        target_slots = list(target_slots)
    seg, _ = _slot_targets(slots, target_slots, None, False)
    B, _C = seg.shape
    T = len(target_slots)
    mask = seg >= 0
    rows = torch.arange(B, dtype=torch.int32, device=seg.device).reshape(-1, 1) * T
    sp = (seg + rows)[mask]
    return mask, sp, B, T, B * T


KEY_NOT_POOLED = -(1 << 63)      # sort key of entries that are not pooled (include/recnow.h, recnow_slot_targets)


class EmbeddingTable(torch.nn.Module):
    """`embedding_func` backed by one dense (V, D) table (the reference docstring's own example, :254-256:
    `tf.nn.embedding_lookup(params, ids)`).  Passing an instance to embedding_using_sparse_batch_segment_ids selects the
    fused path: the pooled rows are gathered straight from the table, no unique/gather round trip."""

    def __init__(self, params, sparse_grad=False):
        """sparse_grad: hand the table's gradient back as a torch.sparse_coo_tensor of the rows that were looked up (what the
        reference path yields: tf.IndexedSlices) instead of a dense, zero-filled (V, D) tensor -- for large tables the dense form is
        hundreds of MB of memset and optimizer traffic per step.  Costs one host sync per backward (the number of distinct ids is
        data-dependent); use with an optimizer that accepts sparse gradients (torch.optim.SparseAdam, SGD)."""
        super().__init__()
        self.weight = params if isinstance(params, torch.nn.Parameter) else torch.nn.Parameter(torch.as_tensor(params, dtype=torch.float32))
        self.sparse_grad = bool(sparse_grad)

    def forward(self, ids):
        _lib.require_gpu(ids, 'ids')
        return _lookup_rows(self.weight, ids.reshape(-1).to(torch.int64)).reshape(tuple(ids.shape) + (self.weight.shape[1],))


class _Sorted(object):
    """Entries sorted by id (lazy: only the backward of a trainable table, or the unique path, needs it)."""

    def __init__(self, key, key32=None):
        self.key = key
        self.key32 = key32          # the same keys as int32 (table path, V < 2^31 - 1): what the sort runs on
        self._seg = None

    def segments(self):
        if self._seg is None:
            self._seg = build_segments((self.key if self.key32 is None else self.key32).reshape(-1))
        return self._seg


class _PoolFunction(torch.autograd.Function):
    """out (B,T,D) = segment-sum/mean over the pooled entries of weights * table[rows].  `table` is either the full
    embedding table (rows = ids; its gradient is scattered into a dense (V,D) tensor) or the (U,D) embeddings of the
    unique ids (rows = inverse index; the gradient comes out dense in unique order)."""

    @staticmethod
    def forward(ctx, table, rows, seg, weights, T, mean, srt, dense_scatter):
        table = _lib.f32c(table, 'embedding table')
        B, C = seg.shape
        D = table.shape[1]
        dev = seg.device
        out = torch.empty((B, T, D), dtype=torch.float32, device=dev)       # every element is written by the kernel
        cnt = torch.empty((B, T), dtype=torch.float32, device=dev) if mean else None
        _lib.call('recnow_embed_pool_fwd', _lib.ptr(table), D, table.shape[0], _lib.ptr(rows), _lib.ptr(seg), _lib.ptr(weights), B, C, T,
                  1 if mean else 0, _lib.ptr(out), _lib.ptr(cnt), _lib.stream())
        need_dw = weights is not None and ctx.needs_input_grad[3]
        ctx.save_for_backward(seg, weights, cnt, *((table, rows) if need_dw else ()))
        ctx.meta = (T, D, bool(mean), srt, dense_scatter, table.shape[0], need_dw)
        return out

    @staticmethod
    def backward(ctx, dout):
        seg, weights, cnt, *extra = ctx.saved_tensors
        T, D, mean, srt, dense_scatter, V, need_dw = ctx.meta
        B, C = seg.shape
        N = B * C
        dev = seg.device
        dout = _lib.f32c(dout, 'grad')
        dweights = None
        if need_dw:             # TF autodiff of `embeddings * expand_dims(sp_weights, -1)` (reference :315-317)
            table, rows = extra
            dweights = torch.empty((B, C), dtype=torch.float32, device=dev)
            _lib.call('recnow_embed_pool_bwd_weights', _lib.ptr(table), D, V, _lib.ptr(rows), _lib.ptr(seg), _lib.ptr(cnt), _lib.ptr(dout),
                      B, C, T, 1 if mean else 0, _lib.ptr(dweights), _lib.stream())
        if not ctx.needs_input_grad[0]:
            return None, None, None, dweights, None, None, None, None
        s = srt.segments()
        drows = torch.empty((max(N, 1), D), dtype=torch.float32, device=dev)
        row_ids = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
        ws = _lib.workspace(_lib.load().recnow_embed_rows_bwd_workspace_bytes(N, D), dev)
        _lib.call('recnow_embed_rows_bwd', _lib.ptr(srt.key), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first),
                  _lib.ptr(s.n_seg), _lib.ptr(seg), _lib.ptr(weights), _lib.ptr(cnt), _lib.ptr(dout), N, C, T, D, 1 if mean else 0,
                  _lib.ptr(drows), _lib.ptr(row_ids), _lib.ptr(ws), ws.numel(), _lib.stream())
        if dense_scatter == 'sparse':
            n_used = s.num_segments()                    # distinct keys (incl. the one "not pooled" key, which sorts last)
            ids = row_ids[:n_used]
            keep = (ids >= 0) & (ids < V)                       # drops the not-pooled key and ids outside the table
            dtable = torch.sparse_coo_tensor(ids[keep].unsqueeze(0), drows[:n_used][keep], (V, D))
        elif dense_scatter:
            dtable = torch.zeros((V, D), dtype=torch.float32, device=dev)
            _lib.call('recnow_embed_scatter_rows', _lib.ptr(drows), _lib.ptr(row_ids), N, D, V, _lib.ptr(dtable), _lib.ptr(s.n_seg), _lib.stream())
        else:
            dtable = drows[:V]                      # unique path: segment s IS unique id s
        return dtable, None, None, dweights, None, None, None, None


def _lookup_rows(table, ids):
    """Plain row lookup table[ids] (EmbeddingTable called directly) = pooling with one entry per output row."""
    n = ids.numel()
    ids2 = ids.reshape(n, 1).contiguous()
    seg = torch.zeros((n, 1), dtype=torch.int32, device=ids.device)
    return _PoolFunction.apply(table, ids2, seg, None, 1, False, _Sorted(ids2), True).reshape(n, table.shape[1])


def embedding_using_sparse_batch_segment_ids(embedding_func, slots, target_slots, ids, weights=None, method='sum', use_unique=True):
    """Embed ids and pool them by slot: out[b][t] = sum (or mean) over the columns c of row b whose slot is
    target_slots[t] of weights[b][c] * embedding(ids[b][c]).

    Args:
        embedding_func: an EmbeddingTable (fused path), or any callable mapping a 1-D int64 id tensor to (n, D) embeddings.
        slots: (B, C) integer slots of the ids;  target_slots: list of T slots to pool;  ids: (B, C) ids (>= 0).
        weights: optional (B, C) per-id weights; differentiable (d out / d weights as TF autodiff gives it).
        method: 'sum' or 'mean';  use_unique: look each distinct id up once (:305-311) - only matters for a callable
            embedding_func, the fused table path never gathers an id it does not pool.
    Returns:
        pooled_embedding (B, T, D).
    """
    if method not in ('sum', 'mean'):
        raise ValueError("method must be 'sum' or 'mean'")
    if not isinstance(target_slots, list):
        target_slots = list(target_slots)
    if not isinstance(ids, torch.Tensor):
        ids = torch.as_tensor(ids, device='cuda')
    _lib.require_gpu(ids, 'ids')
    ids = ids.to(torch.int64).contiguous()
    if weights is not None:
        weights = _lib.f32c(weights, 'weights')
        if weights.shape != ids.shape:
            raise ValueError('weights must have the shape of ids')
    T = len(target_slots)
    if isinstance(embedding_func, EmbeddingTable):
        seg, key, key32 = _slot_targets(slots, target_slots, ids, True, id_limit=int(embedding_func.weight.shape[0]))
    else:
        (seg, key), key32 = _slot_targets(slots, target_slots, ids, True), None
    if seg.shape != ids.shape:
        raise ValueError('slots and ids must have the same (B, C) shape')
    srt = _Sorted(key, key32)
    mean = method == 'mean'
    if isinstance(embedding_func, EmbeddingTable):
        return _PoolFunction.apply(embedding_func.weight, ids, seg, weights, T, mean, srt, 'sparse' if embedding_func.sparse_grad else True)
    B, C = ids.shape
    N = B * C
    dev = ids.device
    if not use_unique:
        # the reference embeds every pooled entry separately (:312-313); entries that are not pooled get id 0's row index
        # but weight in no segment.  Done through the unique path with identity inverse = one lookup per entry.
        emb = embedding_func(torch.where(seg.reshape(-1) >= 0, ids.reshape(-1), torch.zeros_like(ids.reshape(-1))))
        rows = torch.arange(N, dtype=torch.int64, device=dev).reshape(B, C)
        srt_id = _Sorted(torch.where(seg >= 0, rows, torch.full_like(rows, KEY_NOT_POOLED)))
        return _PoolFunction.apply(emb, rows, seg, weights, T, mean, srt_id, True)
    s = srt.segments()
    unique = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
    inverse = torch.empty((B, C), dtype=torch.int64, device=dev)
    n_unique = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call('recnow_embed_unique', _lib.ptr(key), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first), _lib.ptr(s.n_seg), N,
              _lib.ptr(unique), _lib.ptr(inverse), _lib.ptr(n_unique), _lib.stream())
    U = int(n_unique.item())                       # data-dependent size, as tf.unique's output (the one host sync of the path)
    if U < 0:
        s.num_segments()                           # raises: the cooperative grouping kernel timed out (n_seg = -1)
    emb = embedding_func(unique[:U])               # (U, D), ids in ascending order
    if emb.dim() != 2 or emb.shape[0] != U:
        raise ValueError('embedding_func must map n ids to an (n, D) tensor')
    if U == 0:
        emb = emb.new_zeros((1, emb.shape[1] if emb.dim() == 2 else 1))
    return _PoolFunction.apply(emb, inverse, seg, weights, T, mean, srt, False)


def embedding_using_batch_segment_ids(embedding_func, slots, target_slots, ids, weights=None):
    """embedding_util.py:198-215.  The reference's first version of the pooled lookup with method='sum'; the same values, routed to
    embedding_using_sparse_batch_segment_ids (which the reference's docstring tells its users to call instead)."""
    return embedding_using_sparse_batch_segment_ids(embedding_func, slots, target_slots, ids, weights=weights, method='sum', use_unique=True)


def embedding_using_sparse_batch_segment_ids_v1(embedding_func, slots, target_slots, ids, weights=None):
    """embedding_util.py:218-236.  As embedding_using_batch_segment_ids: the pooled lookup with method='sum'."""
    return embedding_using_sparse_batch_segment_ids(embedding_func, slots, target_slots, ids, weights=weights, method='sum', use_unique=True)


# ---- the rest of embedding_util: single-slot fetch, sequence embedding, slot pooling (csrc/slot_fetch.hip) and the small helpers -------------

def _int_tensor(t, what):
    """int32 / int64 GPU tensor, contiguous, dtype kept."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, device='cuda')
    _lib.require_gpu(t, what)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError('%s must be an int32 or int64 tensor, got %s' % (what, t.dtype))
    return t.contiguous(), (_KEY_I64 if t.dtype == torch.int64 else _KEY_I32)


def _single_slot_inputs(slots, target_slot, ids, weights, ncols):
    """Checks shared by fetch_single_slot and embedding_single_slot; everything that can be refused is refused before any launch."""
    if ncols is not None and (int(ncols) != ncols or ncols < 0):
        raise ValueError('ncols must be None or an integer >= 0, got %r' % (ncols,))
    slots, sdt, _ = _slot_tensor(slots)
    if slots.dim() != 2:
        raise ValueError('slots must be a (B, C) matrix')
    idt = _KEY_I64
    if ids is not None:
        ids, idt = _int_tensor(ids, 'ids')
        if ids.shape != slots.shape:
            raise ValueError('slots and ids must have the same (B, C) shape')
    if weights is not None:
        weights = _lib.f32c(weights, 'weights')
        if weights.shape != slots.shape:
            raise ValueError('weights must have the shape of slots')
    return slots, sdt, int(target_slot), ids, idt, weights


def _resolve_ncols(slots, sdt, target, ncols):
    """ncols=None: the largest number of entries of the slot in one row -- ONE host sync (the output shape depends on the data)."""
    if ncols is not None:
        return int(ncols)
    B, C = slots.shape
    mc = torch.empty(1, dtype=torch.int32, device=slots.device)
    _lib.call('recnow_slot_max_count', _lib.ptr(slots), sdt, target, B, C, _lib.ptr(mc), _lib.stream())
    return int(mc.item())


class _FetchFunction(torch.autograd.Function):
    """(target_weights, target_ids) of one slot; differentiable with respect to weights (a copy: the gradient goes back to the source columns)."""

    @staticmethod
    def forward(ctx, weights, slots, sdt, target, ids, idt, ncols, default_id, default_weight):
        B, C = slots.shape
        dev = slots.device
        out_ids = torch.empty((B, ncols), dtype=ids.dtype, device=dev) if ids is not None else None       # every element is written by the kernel
        out_w = torch.empty((B, ncols), dtype=torch.float32, device=dev) if weights is not None else None
        need_dw = weights is not None and ctx.needs_input_grad[0]
        src = torch.empty((B, ncols), dtype=torch.int32, device=dev) if need_dw else None
        if out_ids is not None or out_w is not None:
            _lib.call('recnow_slot_fetch', _lib.ptr(slots), sdt, target, _lib.ptr(ids), idt, _lib.ptr(weights), B, C, ncols, int(default_id),
                      float(default_weight), _lib.ptr(out_ids), _lib.ptr(out_w), None, _lib.ptr(src), _lib.stream())
        if out_ids is not None:
            ctx.mark_non_differentiable(out_ids)
        if need_dw:
            ctx.save_for_backward(src)
        ctx.meta = (B, C, ncols, need_dw)
        return out_w, out_ids

    @staticmethod
    def backward(ctx, dw, _dids):
        B, C, ncols, need_dw = ctx.meta
        if not need_dw or dw is None:
            return (None,) * 9
        return (_fetch_bwd(ctx.saved_tensors[0], dw, B, C, ncols),) + (None,) * 8


def _fetch_bwd(src, dw, B, C, ncols):
    dw = _lib.f32c(dw, 'grad')
    dweights = torch.empty((B, C), dtype=torch.float32, device=dw.device)
    _lib.call('recnow_slot_fetch_bwd', _lib.ptr(src), _lib.ptr(dw), B, C, ncols, _lib.ptr(dweights), _lib.stream())
    return dweights


def fetch_single_slot(slots, target_slot, ids=None, weights=None, default_id=0, default_weight=0, ncols=None):
    """Fetch one slot's ids and weights, padded (or truncated) to ncols columns: embedding_util.py:531-584.

    Row b of each output holds the entries of row b whose slot equals target_slot, in column order; a row with more than ncols of them keeps
    the first ncols, a row with fewer is filled up with default_id / default_weight (RaggedTensor.to_tensor(shape=[nrows, ncols])).

    Args:
        slots: (B, C) integer slots;  target_slot: the slot to fetch;  ids: optional (B, C) int32 / int64 ids (the dtype is kept);
        weights: optional (B, C) weights (fp32; differentiable);  ncols: output columns, None = the largest count of the slot in one row
            (0 if it occurs nowhere: outputs of shape (B, 0)).
    Returns:
        (target_ids (B, ncols) or None, target_weights (B, ncols) or None).

    One HIP kernel (csrc/slot_fetch.hip).  With an explicit ncols there is no host synchronisation and nothing is allocated but the outputs
    (plus a (B, ncols) int32 source-column map when `weights` needs a gradient), so the call can be captured in a graph.  ncols=None costs
    exactly one sync (the maximum count decides the output shape).
    """
    slots, sdt, target, ids, idt, weights = _single_slot_inputs(slots, target_slot, ids, weights, ncols)
    if ids is None and weights is None:
        return None, None
    ncols = _resolve_ncols(slots, sdt, target, ncols)
    out_w, out_ids = _FetchFunction.apply(weights, slots, sdt, target, ids, idt, ncols, default_id, default_weight)
    return out_ids, out_w


class _SlotEmbedFunction(torch.autograd.Function):
    """(embeddings (B, ncols, D), weights (B, ncols), mask (B, ncols)) of one slot.  `table` is the embedding table (rows = the ids) or the (U, D)
    embeddings a callable returned (rows = the index of each entry's embedding); either way its gradient is the sorted-segment reduction of
    csrc/embed.hip over the B * ncols output positions."""

    @staticmethod
    def forward(ctx, table, weights, rows, rdt, slots, sdt, target, ncols, default_weight, sparse):
        table = _lib.f32c(table, 'embedding table')
        B, C = slots.shape
        V, D = table.shape
        dev = slots.device
        out = torch.empty((B, ncols, D), dtype=torch.float32, device=dev)                                  # every element is written by the kernel
        out_w = torch.empty((B, ncols), dtype=torch.float32, device=dev) if weights is not None else None
        mask = torch.empty((B, ncols), dtype=torch.bool, device=dev)
        need_dt = ctx.needs_input_grad[0] and V > 0
        need_dw = weights is not None and ctx.needs_input_grad[1]
        narrow = V < (1 << 31) - 1
        key = torch.empty((B, ncols), dtype=torch.int64, device=dev) if need_dt else None
        key32 = torch.empty((B, ncols), dtype=torch.int32, device=dev) if need_dt and narrow else None
        src = torch.empty((B, ncols), dtype=torch.int32, device=dev) if need_dw else None
        _lib.call('recnow_slot_embed_fwd', _lib.ptr(table), D, V, _lib.ptr(slots), sdt, target, _lib.ptr(rows), rdt, _lib.ptr(weights), B, C, ncols,
                  float(default_weight), _lib.ptr(out), _lib.ptr(out_w), _lib.ptr(mask), _lib.ptr(src), _lib.ptr(key), _lib.ptr(key32),
                  max(V, 1), _lib.stream())
        ctx.mark_non_differentiable(mask)
        ctx.save_for_backward(key, key32, src)
        ctx.meta = (B, C, ncols, V, D, need_dt, need_dw, sparse)
        return out, out_w, mask

    @staticmethod
    def backward(ctx, dout, dw, _dmask):
        key, key32, src = ctx.saved_tensors
        B, C, ncols, V, D, need_dt, need_dw, sparse = ctx.meta
        dweights = _fetch_bwd(src, dw, B, C, ncols) if need_dw and dw is not None else None
        dtable = None
        if need_dt and dout is not None:
            dout = _lib.f32c(dout, 'grad')
            dev = dout.device
            N = B * ncols
            if N == 0:
                dtable = torch.sparse_coo_tensor(torch.empty((1, 0), dtype=torch.int64, device=dev), torch.empty((0, D), device=dev), (V, D)) \
                    if sparse else torch.zeros((V, D), dtype=torch.float32, device=dev)
            else:
                s = build_segments((key if key32 is None else key32).reshape(-1))
                ws = _lib.workspace(_lib.load().recnow_embed_rows_bwd_workspace_bytes(N, D), dev)
                if sparse:              # as _PoolFunction: the rows that were looked up, one host sync for their number
                    drows = torch.empty((N, D), dtype=torch.float32, device=dev)
                    row_ids = torch.empty(N, dtype=torch.int64, device=dev)
                    live = -(key.reshape(-1) >= V).to(torch.int32)             # 0: a table row, -1: padding / outside the table (no gradient)
                    _lib.call('recnow_embed_rows_bwd', _lib.ptr(key), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first), _lib.ptr(s.n_seg),
                              _lib.ptr(live), None, None, _lib.ptr(dout), N, 1, 1, D, 0, _lib.ptr(drows), _lib.ptr(row_ids), _lib.ptr(ws), ws.numel(),
                              _lib.stream())
                    n_used = s.num_segments()
                    rid = row_ids[:n_used]
                    keep = (rid >= 0) & (rid < V)
                    dtable = torch.sparse_coo_tensor(rid[keep].unsqueeze(0), drows[:n_used][keep], (V, D))
                else:
                    dtable = torch.zeros((V, D), dtype=torch.float32, device=dev)
                    _lib.call('recnow_embed_rows_bwd_direct', _lib.ptr(key), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first),
                              _lib.ptr(s.n_seg), None, 1, _lib.ptr(dout), N, 1, D, _lib.ptr(dtable), V, _lib.ptr(ws), ws.numel(), _lib.stream())
        return (dtable, dweights) + (None,) * 8


def embedding_single_slot(embedding_func, slots, target_slot, ids, weights=None, default_weight=0, ncols=None, use_unique=True):
    """One slot's embeddings WITHOUT pooling -- a sequence, e.g. the click history attention_by_dot_product / attention_by_dnn take as
    user_emb: embedding_util.py:327-416.

    Args:
        embedding_func: an EmbeddingTable (fused path: selection and gather are one kernel), or any callable mapping a 1-D int64 id tensor to
            (n, D) embeddings;
        slots: (B, C) integer slots;  target_slot: the slot to embed;  ids: (B, C) int32 / int64 ids;  weights: optional (B, C) weights;
        default_weight: weight of the padding positions;  ncols: sequence length (rows are truncated / padded to it), None = the largest
            count of the slot in one row;  use_unique: a callable sees every distinct selected id once, in ascending order (True), or the
            selected ids in row-major order (False).  The table path never gathers an id it does not output.
    Returns:
        embedding_tensor (B, ncols, D) fp32, zero rows at padding;  weights_tensor (B, ncols, 1) or None;  mask_tensor (B, ncols, 1) bool,
        False at padding.

    Gradients reach the table (dense, or a torch.sparse_coo_tensor with EmbeddingTable(sparse_grad=True)), a callable's output and `weights`.
    An id outside [0, V) on the table path reads as a zero row and gets no gradient, as in the pooled lookup; its mask entry is True.
    Host synchronisation: the table path with an explicit ncols has none in the forward and allocates only its outputs (plus the int32 / int64
    sort keys and source columns of the (B, ncols) positions when a gradient is wanted); ncols=None adds exactly one (the maximum count).  The
    callable path synchronises once more for the number of ids handed to the callable (tf.unique / boolean_mask have data-dependent sizes),
    and use_unique=False compacts the ids with a few torch ops (API parity, not a hot path).  The dense table gradient is bit-identical from
    run to run; the positions B * ncols must stay below 2^31.
    """
    if ids is None:
        raise ValueError('embedding_single_slot needs ids')
    slots, sdt, target, ids, idt, weights = _single_slot_inputs(slots, target_slot, ids, weights, ncols)
    ncols = _resolve_ncols(slots, sdt, target, ncols)
    B, C = slots.shape
    dev = slots.device
    if isinstance(embedding_func, EmbeddingTable):
        table, rows, rdt, sparse = embedding_func.weight, ids, idt, embedding_func.sparse_grad
    elif use_unique:
        sparse, rdt = False, _KEY_I64
        _seg, key = _slot_targets(slots, [target], ids.to(torch.int64), True)
        N = B * C
        s = build_segments(key.reshape(-1))
        unique = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
        rows = torch.empty((B, C), dtype=torch.int64, device=dev)
        n_unique = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call('recnow_embed_unique', _lib.ptr(key), _lib.ptr(s.order), _lib.ptr(s.seg_id), _lib.ptr(s.seg_first), _lib.ptr(s.n_seg), N,
                  _lib.ptr(unique), _lib.ptr(rows), _lib.ptr(n_unique), _lib.stream())
        U = int(n_unique.item())                       # data-dependent size, as tf.unique's output
        if U < 0:
            s.num_segments()                           # raises: the cooperative grouping kernel timed out
        table = embedding_func(unique[:U])
        if table.dim() != 2 or table.shape[0] != U:
            raise ValueError('embedding_func must map n ids to an (n, D) tensor')
    else:
        sparse, rdt = False, _KEY_I64
        sel = slots == target
        flat = sel.reshape(-1)
        rows = (torch.cumsum(flat, 0) - 1).reshape(B, C)                    # entry -> its place among the selected entries, row-major
        picked = ids.reshape(-1)[flat].to(torch.int64)                      # data-dependent size, as tf.boolean_mask's output
        table = embedding_func(picked)
        if table.dim() != 2 or table.shape[0] != picked.numel():
            raise ValueError('embedding_func must map n ids to an (n, D) tensor')
    out, out_w, mask = _SlotEmbedFunction.apply(table, weights, rows, rdt, slots, sdt, target, ncols, default_weight, sparse)
    return out, (out_w.unsqueeze(-1) if out_w is not None else None), mask.unsqueeze(-1)


class _SlotPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, seg, ids, idt, T, mean, drop):
        B, C = seg.shape
        dev = seg.device
        out_ids = torch.empty((B, T), dtype=ids.dtype, device=dev) if ids is not None else None            # every element is written by the kernel
        out_w = torch.empty((B, T), dtype=torch.float32, device=dev) if weights is not None else None
        need_dw = weights is not None and ctx.needs_input_grad[0]
        cnt = torch.empty((B, T), dtype=torch.float32, device=dev) if need_dw and mean else None
        _lib.call('recnow_slot_pool_fwd', _lib.ptr(seg), _lib.ptr(ids), idt, _lib.ptr(weights), B, C, T, 1 if mean else 0, 1 if drop else 0,
                  _lib.ptr(out_ids), _lib.ptr(out_w), _lib.ptr(cnt), _lib.stream())
        if out_ids is not None:
            ctx.mark_non_differentiable(out_ids)
        if need_dw:
            ctx.save_for_backward(seg, cnt)
        ctx.meta = (B, C, T, mean, drop, need_dw)
        return out_w, out_ids

    @staticmethod
    def backward(ctx, dw, _dids):
        B, C, T, mean, drop, need_dw = ctx.meta
        if not need_dw or dw is None:
            return (None,) * 7
        seg, cnt = ctx.saved_tensors
        dw = _lib.f32c(dw, 'grad')
        dweights = torch.empty((B, C), dtype=torch.float32, device=dw.device)
        _lib.call('recnow_slot_pool_bwd', _lib.ptr(seg), _lib.ptr(cnt), _lib.ptr(dw), B, C, T, 1 if mean else 0, 1 if drop else 0,
                  _lib.ptr(dweights), _lib.stream())
        return (dweights,) + (None,) * 6


def pool_slots(slots, target_slots, ids=None, weights=None, method='sum', drop_duplicate_slot=False):
    """Fetch a list of slots at once, one id and one weight per (row, slot): embedding_util.py:419-489.

    Args:
        slots: (B, C) integer slots (1-D: one row);  target_slots: the T slots to pool;  ids: optional int32 / int64 ids of the shape of slots;
        weights: optional weights of that shape (differentiable);  method: 'sum' or 'mean' of the weights;
        drop_duplicate_slot: as the reference, first_occurance_in_row(batch_segment_ids, need_sort=False, padding_value=-1): an entry is dropped
            when the column IMMEDIATELY BEFORE it belongs to the same target slot (equal slots that are not adjacent are all kept).
    Returns:
        pooled_ids (B, T): the smallest id of each slot's entries, 0 where there is none (or where it equals the dtype's maximum);
        pooled_weights (B, T): the sum / mean of their weights, 0 where there is none.  None for an input that is None.

    Two HIP launches (slot -> target index, then one wave per row), no host synchronisation; besides the outputs only the (B, C) int32 target
    index map is allocated (and the (B, T) counts when 'mean' needs a gradient).  Sums add in ascending column order: no atomics.
    """
    target_slots = list(target_slots)
    if method not in ('sum', 'mean'):
        raise ValueError("not support '%s'" % (method,))
    listed = not isinstance(slots, torch.Tensor)
    if listed:
        slots = torch.as_tensor(slots)
    if slots.dim() == 1:
        slots = slots.reshape(1, -1)
    if slots.dim() != 2:
        raise ValueError('only support 2 (or 1) dimentional slots, get %d' % slots.dim())
    if len(set(target_slots)) != len(target_slots):
        raise ValueError('target_slots must not contain duplicates')
    if listed:
        slots = slots.to('cuda')
    _lib.require_gpu(slots, 'slots')
    idt = _KEY_I64
    if ids is not None:
        ids, idt = _int_tensor(ids, 'ids')
        if ids.numel() != slots.numel() or (ids.dim() == 2 and ids.shape != slots.shape):
            raise ValueError('slots and ids must have the same shape')
        ids = ids.reshape(slots.shape)
    if weights is not None:
        weights = _lib.f32c(weights, 'weights')
        if weights.numel() != slots.numel() or (weights.dim() == 2 and weights.shape != slots.shape):
            raise ValueError('weights must have the shape of slots')
        weights = weights.reshape(slots.shape)
    if ids is None and weights is None:
        return None, None
    seg, _ = _slot_targets(slots, target_slots, None, False)
    out_w, out_ids = _SlotPoolFunction.apply(weights, seg, ids, idt, len(target_slots), method == 'mean', bool(drop_duplicate_slot))
    return out_ids, out_w


def pool_single_slot(slots, target_slot, ids=None, weights=None):
    """embedding_util.py:492-528: the entries of one slot as (n, 1) columns -- right only for a slot that occurs exactly once in every row;
    use fetch_single_slot instead (the reference warns in the same words).  API parity on a few torch ops, not a hot path; the boolean mask
    has a data-dependent size, so this function synchronises."""
    warnings.warn("pool_single_slot only work for slot that occur exactly once a sample, use fetch_single_slot instead")
    slots, _sdt, _ = _slot_tensor(slots)
    mask = slots == int(target_slot)

    def fetch(values, what):
        if values is None:
            return None
        if not isinstance(values, torch.Tensor):
            values = torch.as_tensor(values, device='cuda')
        _lib.require_gpu(values, what)
        if values.shape != slots.shape:
            raise ValueError('%s must have the shape of slots' % what)
        return values[mask].reshape(-1, 1)
    return fetch(ids, 'ids'), fetch(weights, 'weights')


def _targets_of(values, target_values):
    """(tensor, seg of its flattened entries as a (1, n) map) through recnow_slot_targets; a repeated target value is looked up once."""
    if not isinstance(values, torch.Tensor):
        values = torch.as_tensor(values, device='cuda')
    _lib.require_gpu(values, 'values')
    seg, _ = _slot_targets(values.reshape(1, -1), list(dict.fromkeys(target_values)), None, False)
    return values, seg.reshape(values.shape)


def isin(values, target_values):
    """Like np.isin for an integer GPU tensor of any shape: embedding_util.py:11-35.  One launch of recnow_slot_targets, no sync."""
    return _targets_of(values, target_values)[1] >= 0


def mask_values(values, target_values, padding_value=0):
    """Keep the values that are in target_values, set the others to padding_value: embedding_util.py:38-50.  No sync."""
    values, seg = _targets_of(values, target_values)
    return torch.where(seg >= 0, values, torch.full_like(values, padding_value))


def first_occurance_in_row(mat, need_sort=False, padding_value=0):
    """Keep a number where it differs from its left neighbour in the row, set it to padding_value otherwise: embedding_util.py:53-82
    (need_sort=True sorts each row first, which makes that "the first occurrence").  API parity on a few torch ops, no sync."""
    listed = not isinstance(mat, torch.Tensor)
    if listed:
        mat = torch.as_tensor(mat)
    if mat.dim() != 2:
        raise ValueError('mat must be 2D tensor, get %dD tensor' % mat.dim())
    if listed:
        mat = mat.to('cuda')
    _lib.require_gpu(mat, 'mat')
    if need_sort:
        mat = torch.sort(mat, dim=-1).values
    right = torch.where(mat[:, :-1] != mat[:, 1:], mat[:, 1:], torch.full_like(mat[:, 1:], padding_value))
    return torch.cat([mat[:, 0:1], right], dim=-1)


def batch_segment_ids_of_targets(slots, target_slots):
    """embedding_util.py:85-134.  Returns (batch_segment_ids (B, C) int32 = row * T + target index, -1 for slots that are no target, num_rows,
    num_ids, num_segments) -- the dense form of sparse_batch_segment_ids_of_targets.  recnow_slot_targets plus two torch ops, no sync."""
    if not isinstance(target_slots, list):
        target_slots = list(target_slots)
    seg, _ = _slot_targets(slots, target_slots, None, False)
    B, _C = seg.shape
    T = len(target_slots)
    rows = torch.arange(B, dtype=torch.int32, device=seg.device).reshape(-1, 1) * T
    return torch.where(seg >= 0, seg + rows, seg), B, T, B * T

"""Independent numpy restatement of the op sequence of the reference's rec_block/embedding_util.py for the single-slot fetch, the sequence
embedding, slot pooling and the small helpers -- tf.boolean_mask (row-major), RaggedTensor.from_value_rowids(...).to_tensor(shape=...) (pad or
truncate), tf.math.unsorted_segment_min / _sum / _mean (negative segment ids dropped), first_occurance_in_row -- and fp64 gradients of the
differentiable outputs.  Nothing here shares code with rec_now_amd."""
import numpy as np


# ---- the TensorFlow ops the reference is written in ------------------------------------------------------------------------------------------
def boolean_mask(values, mask):
    """tf.boolean_mask of a matrix by a matrix mask: the selected entries in row-major order."""
    return np.asarray(values)[np.asarray(mask, dtype=bool)]


def where_rows(mask):
    """tf.where(mask)[:, 0]: the row of every True entry, row-major."""
    return np.nonzero(np.asarray(mask, dtype=bool))[0]


def ragged_to_tensor(values, row_ids, nrows, ncols, default):
    """RaggedTensor.from_value_rowids(values, row_ids).to_tensor(default_value=default, shape=(nrows, ncols) + values.shape[1:]): row r holds the
    values whose row id is r in their order, cut to ncols or filled up with `default`.  ncols=None: the longest row."""
    values = np.asarray(values)
    counts = np.bincount(row_ids, minlength=nrows) if len(row_ids) else np.zeros(nrows, dtype=np.int64)
    if ncols is None:
        ncols = int(counts.max()) if nrows else 0
    out = np.full((nrows, ncols) + values.shape[1:], default, dtype=values.dtype)
    fill = np.zeros(nrows, dtype=np.int64)
    for v, r in zip(values, row_ids):
        if fill[r] < ncols:
            out[r, fill[r]] = v
        fill[r] += 1
    return out


def unsorted_segment(values, segment_ids, num_segments, how):
    """tf.math.unsorted_segment_min / _sum / _mean over flattened inputs; entries with a negative segment id are dropped.  An empty segment is the
    dtype's maximum for min, 0 for sum and mean."""
    values, segment_ids = np.asarray(values).reshape(-1), np.asarray(segment_ids).reshape(-1)
    if how == 'min':
        out = np.full(num_segments, np.iinfo(values.dtype).max, dtype=values.dtype)
    else:
        out = np.zeros(num_segments, dtype=np.float64)
    cnt = np.zeros(num_segments, dtype=np.int64)
    for v, s in zip(values, segment_ids):
        if s < 0:
            continue
        cnt[s] += 1
        if how == 'min':
            out[s] = min(out[s], v)
        else:
            out[s] += float(v)
    if how == 'mean':
        out = out / np.maximum(cnt, 1)
    return out


# ---- the helpers -----------------------------------------------------------------------------------------------------------------------------
def isin(values, target_values):
    return np.isin(np.asarray(values), list(target_values))


def mask_values(values, target_values, padding_value=0):
    values = np.asarray(values)
    return np.where(isin(values, target_values), values, padding_value).astype(values.dtype)


def first_occurance_in_row(mat, need_sort=False, padding_value=0):
    mat = np.asarray(mat)
    if need_sort:
        mat = np.sort(mat, axis=-1)
    right = np.where(mat[:, :-1] != mat[:, 1:], mat[:, 1:], padding_value)
    return np.concatenate([mat[:, 0:1], right], axis=-1).astype(mat.dtype)


def batch_segment_ids_of_targets(slots, target_slots):
    slots = np.asarray(slots)
    table = {s: i for i, s in enumerate(target_slots)}
    seg = np.array([[table.get(int(s), -1) for s in row] for row in slots], dtype=np.int32).reshape(slots.shape)
    nrows, nids = slots.shape[0], len(target_slots)
    shift = nids * np.arange(nrows, dtype=np.int32).reshape(-1, 1) * (seg >= 0)
    return seg + shift, nrows, nids, nids * nrows


# ---- fetch_single_slot / embedding_single_slot -----------------------------------------------------------------------------------------------
def fetch_single_slot(slots, target_slot, ids=None, weights=None, default_id=0, default_weight=0, ncols=None):
    slots = np.asarray(slots)
    mask = slots == target_slot
    row_ids, nrows = where_rows(mask), slots.shape[0]

    def fetch(values, default):
        if values is None:
            return None
        return ragged_to_tensor(boolean_mask(values, mask), row_ids, nrows, ncols, default)
    return fetch(ids, default_id), fetch(weights, default_weight)


def embedding_single_slot(embedding_func, slots, target_slot, ids, weights=None, default_weight=0, ncols=None, use_unique=True):
    """embedding_func: ids -> (n, D) rows.  Returns (embedding_tensor, weights_tensor or None, mask_tensor)."""
    slots = np.asarray(slots)
    mask = slots == target_slot
    row_ids, nrows = where_rows(mask), slots.shape[0]
    sp_ids = boolean_mask(ids, mask)
    if use_unique:
        unique_ids, flat = np.unique(sp_ids, return_inverse=True)
        emb = np.asarray(embedding_func(unique_ids))[flat.reshape(-1)]
    else:
        emb = np.asarray(embedding_func(sp_ids))
    emb_t = ragged_to_tensor(emb, row_ids, nrows, ncols, 0)
    w_t = None
    if weights is not None:
        w_t = ragged_to_tensor(boolean_mask(weights, mask), row_ids, nrows, ncols, default_weight)[..., None]
    m_t = ragged_to_tensor(np.ones(len(row_ids), dtype=bool), row_ids, nrows, ncols, False)[..., None]
    return emb_t, w_t, m_t


def table_lookup(table):
    """embedding_func of a dense table; an id outside the table reads as a zero row (tf.nn.embedding_lookup on a GPU)."""
    table = np.asarray(table)

    def f(ids):
        ids = np.asarray(ids).astype(np.int64)
        ok = (ids >= 0) & (ids < table.shape[0])
        out = np.zeros((len(ids), table.shape[1]), dtype=table.dtype)
        out[ok] = table[ids[ok]]
        return out
    return f


def positions(slots, target_slot, ncols):
    """(B, ncols) source column of every output position, -1 for padding (derived from the ragged layout of the column numbers)."""
    slots = np.asarray(slots)
    cols = np.broadcast_to(np.arange(slots.shape[1], dtype=np.int64), slots.shape)
    src, _ = fetch_single_slot(slots, target_slot, ids=cols, default_id=-1, ncols=ncols)
    return src


def embedding_single_slot_grads(V, slots, target_slot, ids, ncols, d_emb, d_w=None):
    """fp64 gradients of sum(embedding_tensor * d_emb) + sum(weights_tensor * d_w): (d table (V, D), d weights (B, C) or None)."""
    slots, ids = np.asarray(slots), np.asarray(ids)
    src = positions(slots, target_slot, ncols)
    d_emb = np.asarray(d_emb, dtype=np.float64)
    dtable = np.zeros((V, d_emb.shape[-1]), dtype=np.float64)
    dweights = np.zeros(slots.shape, dtype=np.float64) if d_w is not None else None
    for b in range(src.shape[0]):
        for j in range(src.shape[1]):
            c = src[b, j]
            if c < 0:
                continue
            i = int(ids[b, c])
            if 0 <= i < V:
                dtable[i] += d_emb[b, j]
            if dweights is not None:
                dweights[b, c] += float(np.asarray(d_w).reshape(src.shape)[b, j])
    return dtable, dweights


# ---- pool_slots / pool_single_slot -----------------------------------------------------------------------------------------------------------
def pool_slots(slots, target_slots, ids=None, weights=None, method='sum', drop_duplicate_slot=False):
    target_slots = list(target_slots)
    slots = np.asarray(slots)
    if slots.ndim == 1:
        slots = slots.reshape(1, -1)
    seg, nrows, nids, nseg = batch_segment_ids_of_targets(slots, target_slots)

    def pool(values, how):
        if values is None:
            return None
        s = first_occurance_in_row(seg, need_sort=False, padding_value=-1) if drop_duplicate_slot else seg
        if how == 'min0':
            r = unsorted_segment(values, s, nseg, 'min')
            r = np.where(r != np.iinfo(r.dtype).max, r, 0).astype(r.dtype)
        else:
            r = unsorted_segment(values, s, nseg, how)
        return r.reshape(nrows, nids)
    return pool(ids, 'min0'), pool(weights, method)


def pool_slots_weight_grad(slots, target_slots, method, drop_duplicate_slot, d_out):
    """fp64 d sum(pooled_weights * d_out) / d weights."""
    slots = np.asarray(slots)
    seg, nrows, nids, nseg = batch_segment_ids_of_targets(slots, list(target_slots))
    s = first_occurance_in_row(seg, need_sort=False, padding_value=-1) if drop_duplicate_slot else seg
    cnt = np.bincount(s[s >= 0], minlength=nseg)
    g = np.asarray(d_out, dtype=np.float64).reshape(-1)
    out = np.zeros(slots.shape, dtype=np.float64)
    keep = s >= 0
    out[keep] = g[s[keep]] / (np.maximum(cnt, 1)[s[keep]] if method == 'mean' else 1.0)
    return out


def pool_single_slot(slots, target_slot, ids=None, weights=None):
    mask = np.asarray(slots) == target_slot
    f = lambda v: None if v is None else boolean_mask(v, mask).reshape(-1, 1)      # noqa: E731
    return f(ids), f(weights)


def calc_sum_of_abs_diff(a, b):
    """The reference tests' criterion (rec_now/util/numpy_tools.py)."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).sum())

"""fp64 oracles of the pooled-embedding kernels (rec_now_amd/csrc/embed.hip), one per entry point, written from the header comments of the
kernels and from nothing else of them: no chunks, no sorted order, no joins.  numpy only.

The summing oracles also return, per output element, the number of terms n and sum |term|.  An fp32 sum of n rounded products passes every
term through at most one product rounding and n - 1 additions, in any association: it is within n 2^-24 sum |term| of the exact sum to first
order, and the division of 'mean' adds one more rounding -- bound(n, sabs) below is the (n + 2) 2^-24 sum |term| the GPU tests hold every
element to.
"""
import numpy as np

U32 = 2.0 ** -24


def bound(n, sabs):
    n = np.asarray(n, np.float64)
    return (n.reshape(n.shape + (1,) * (np.ndim(sabs) - n.ndim)) + 2.0) * U32 * sabs


def pool_fwd(table, rows, seg, weights, T, mean):
    """out[b][t][:] = sum over the columns c of row b with seg[b][c] == t of w[b][c] * table[rows[b][c]][:], / cnt[b][t] for mean.  A row index
    outside [0, V) is a zero row that still counts; an empty target gives 0.  -> out (B, T, D), cnt (B, T), n (B, T), sabs (B, T, D)"""
    table = np.asarray(table, np.float64)
    V, D = table.shape
    B, C = seg.shape
    out, sabs = np.zeros((B, T, D)), np.zeros((B, T, D))
    cnt = np.zeros((B, T), np.int64)
    for b in range(B):
        for c in range(C):
            t = int(seg[b, c])
            if t < 0:
                continue
            cnt[b, t] += 1
            r = int(rows[b, c])
            if 0 <= r < V:
                term = (1.0 if weights is None else float(weights[b, c])) * table[r]
                out[b, t] += term
                sabs[b, t] += np.abs(term)
    if mean:
        d = np.maximum(cnt, 1)[:, :, None]
        out, sabs = out / d, sabs / d
    return out, cnt.astype(np.float64), cnt, sabs


def _coef(e, t, w, cnt, C, T, mean):
    b = e // C
    coef = np.ones(e.shape, np.float64) if w is None else np.asarray(w, np.float64)[e]
    if mean:
        coef = coef / np.asarray(cnt, np.float64).reshape(-1)[b * T + t]
    return b, coef


def rows_bwd(key, t, weights, cnt, dout, C, mean):
    """Per distinct key: sum over the entries e with that key of w_e * dout[e // C][t_e][:] (/ cnt[e // C][t_e] for mean); entries with t < 0
    add nothing.  -> keys (U,) ascending as signed numbers, sums (U, D), n (U,) contributing entries, sabs (U, D)"""
    key, t = np.asarray(key, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1)
    dout = np.asarray(dout, np.float64)
    _, T, D = dout.shape
    keys, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    e = np.flatnonzero(t >= 0)
    b, coef = _coef(e, t[e], weights, cnt, C, T, mean)
    terms = coef[:, None] * dout[b, t[e]]                       # (n_pooled, D)
    srt = np.argsort(inv[e], kind='stable')
    sums, sabs = np.zeros((len(keys), D)), np.zeros((len(keys), D))
    n = np.bincount(inv[e], minlength=len(keys))
    if len(e):
        starts = np.flatnonzero(np.diff(inv[e][srt], prepend=-1))
        present = inv[e][srt][starts]
        sums[present] = np.add.reduceat(terms[srt], starts, axis=0)
        sabs[present] = np.add.reduceat(np.abs(terms[srt]), starts, axis=0)
    return keys, sums, n, sabs


def rows_bwd_dense(key, t, weights, cnt, dout, C, mean):
    """the same as rows_bwd, entry by entry into a dense array (np.add.at): the independent formulation the CPU test holds rows_bwd to"""
    key, t = np.asarray(key, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1)
    dout = np.asarray(dout, np.float64)
    _, T, D = dout.shape
    keys = np.array(sorted(set(key.tolist())), np.int64)
    slot = {k: i for i, k in enumerate(keys.tolist())}
    sums, sabs, n = np.zeros((len(keys), D)), np.zeros((len(keys), D)), np.zeros(len(keys), np.int64)
    pooled = [e for e in range(len(key)) if t[e] >= 0]
    idx = np.array([slot[int(key[e])] for e in pooled], np.int64)
    terms = np.zeros((len(pooled), D))
    for i, e in enumerate(pooled):
        b = e // C
        c = 1.0 if weights is None else float(weights[e])
        if mean:
            c = c / float(np.asarray(cnt)[b, t[e]])
        terms[i] = c * dout[b, t[e]]
    np.add.at(sums, idx, terms)
    np.add.at(sabs, idx, np.abs(terms))
    np.add.at(n, idx, 1)
    return keys, sums, n, sabs


def rows_bwd_direct(key, weights, w_div, dout, C, V):
    """dtable[key][:] = sum over the entries e of that key of weights[e // w_div] * dout[e // C][:]; keys outside [0, V) are dropped.
    -> dtable (V, D), n (V,), sabs (V, D), named (V,) bool: rows some key names"""
    key = np.asarray(key, np.int64).reshape(-1)
    dout = np.asarray(dout, np.float64)
    D = dout.shape[-1]
    w = None if weights is None else np.asarray(weights, np.float64)[np.arange(len(key)) // w_div]
    keys, sums, n, sabs = rows_bwd(key, np.zeros(len(key), np.int64), w, None, dout.reshape(-1, 1, D), C, False)
    ok = (keys >= 0) & (keys < V)
    dt, sa, nn, named = np.zeros((V, D)), np.zeros((V, D)), np.zeros(V, np.int64), np.zeros(V, bool)
    dt[keys[ok]], sa[keys[ok]], nn[keys[ok]], named[keys[ok]] = sums[ok], sabs[ok], n[ok], True
    return dt, nn, sa, named


def pool_bwd_weights(table, rows, seg, cnt, dout, mean):
    """dweights[b][c] = <dout[b][seg[b][c]][:], table[rows[b][c]][:]> (/ cnt for mean); 0 for entries that are not pooled and for rows outside
    the table.  -> dweights (B, C), sabs (B, C); every element is a sum of D terms"""
    table, dout = np.asarray(table, np.float64), np.asarray(dout, np.float64)
    V = table.shape[0]
    B, C = seg.shape
    dw, sabs = np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        for c in range(C):
            t, r = int(seg[b, c]), int(rows[b, c])
            if t < 0 or not 0 <= r < V:
                continue
            p = dout[b, t] * table[r]
            d = float(cnt[b, t]) if mean else 1.0
            if d > 0:
                dw[b, c], sabs[b, c] = p.sum() / d, np.abs(p).sum() / d
    return dw, sabs


def embed_unique(key, order, lengths, sentinel):
    """unique[s] = the key of sorted segment s, inverse[entry] = its segment, n_unique = the number of segments, less the last one if that is
    the sentinel segment.  -> unique (S,), inverse (N,), n_unique"""
    key = np.asarray(key, np.int64).reshape(-1)
    S = len(lengths)
    unique, inverse = np.zeros(S, np.int64), np.zeros(len(key), np.int64)
    k = 0
    for s, n in enumerate(lengths):
        ent = order[k:k + n]
        assert len(set(key[ent].tolist())) == 1
        unique[s] = key[ent[0]]
        inverse[ent] = s
        k += n
    return unique, inverse, S - 1 if S and unique[-1] == sentinel else S


def scatter_rows(drows, row_ids, n_slots, V, n_seg=None, fill=np.nan):
    """dtable[row_ids[s]] = drows[s] for the slots s < n_slots (< n_seg where a count 0 <= n_seg < n_slots is given) whose id is a row of the
    table; every other row of dtable keeps `fill`.  -> dtable (V, D), written (V,) bool"""
    drows = np.asarray(drows)
    dt = np.full((V, drows.shape[1]), fill, drows.dtype)
    written = np.zeros(V, bool)
    if n_seg is not None and 0 <= n_seg < n_slots:
        n_slots = n_seg
    for s in range(n_slots):
        r = int(row_ids[s])
        if 0 <= r < V:
            assert not written[r], 'row ids are unique'
            dt[r], written[r] = drows[s], True
    return dt, written

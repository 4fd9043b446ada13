"""fp64 oracle of attention_by_softmax and of TargetAttentionLayer (in its UNFOLDED form: every position is projected), written as the loops
of the definitions -- per sample, head and position -- plus the input generator, the shapes and the error measures that
tests/test_attention_softmax_cpu.py and tests/test_attention_softmax_gpu.py share.

    K(b) = { l : l < lengths[b] and mask[b, l] != 0 }
    s_hl = scale <q[b,h], x[b,l]>,  a_hl = exp(s_hl - max) / sum over K(b),  out[b,h] = sum_l a_hl x[b,l],  lse[b,h] = log sum exp(s_hl)
    ds_hl = a_hl (<dc_h, x_l> - <dc_h, out_h>),  dx_l = sum_h (a_hl dc_h + scale ds_hl q_h),  dq_h = scale sum_l ds_hl x_l

A sample without a key: out = 0, lse = -inf, no gradient.  Positions outside K(b) are never read (they may hold anything)."""
import functools
import math

import numpy as np

TOL = 1e-5          # per row: TOL * max(1, largest |reference| entry of the row)
TOL_LSE = 1e-6      # per entry: TOL_LSE * max(1, |lse|)
MODES = ('none', 'lengths', 'mask', 'both')


def keys_of(B, L, lengths=None, mask=None):
    """(B, L) bool: position l is a key of sample b."""
    k = np.ones((B, L), dtype=bool)
    if lengths is not None:
        n = np.clip(np.asarray(lengths).reshape(-1).astype(np.int64), 0, L)
        k &= np.arange(L)[None, :] < n[:, None]
    if mask is not None:
        k &= np.asarray(mask).reshape(B, L) != 0
    return k


def run(x, q, lengths=None, mask=None, scale=None, dc=None):
    """x (B, L, D), q (B, H, D), dc (B, H, D) or None -> dict(out (B, H, D), lse (B, H), a (B, H, L), ds (B, H, L), dx, dq), all fp64."""
    x64, q64 = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    B, L, D = x64.shape
    H = q64.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    key = keys_of(B, L, lengths, mask)
    out, lse = np.zeros((B, H, D)), np.full((B, H), -np.inf)
    a, ds = np.zeros((B, H, L)), np.zeros((B, H, L))
    dx, dq = np.zeros((B, L, D)), np.zeros((B, H, D))
    dc64 = None if dc is None else np.asarray(dc, dtype=np.float64)
    for b in range(B):
        ls = [l for l in range(L) if key[b, l]]
        if not ls:
            continue
        for h in range(H):
            s = {l: scale * float(np.dot(q64[b, h], x64[b, l])) for l in ls}
            top = max(s.values())
            total = 0.0
            for l in ls:
                total += math.exp(s[l] - top)
            lse[b, h] = top + math.log(total)
            for l in ls:
                a[b, h, l] = math.exp(s[l] - top) / total
                out[b, h] += a[b, h, l] * x64[b, l]
            if dc64 is None:
                continue
            gbar = float(np.dot(dc64[b, h], out[b, h]))
            for l in ls:
                d = a[b, h, l] * (float(np.dot(dc64[b, h], x64[b, l])) - gbar)
                ds[b, h, l] = d
                dx[b, l] += a[b, h, l] * dc64[b, h] + (scale * d) * q64[b, h]
                dq[b, h] += (scale * d) * x64[b, l]
    return dict(out=out, lse=lse, a=a, ds=ds, dx=dx, dq=dq, key=key)


def run_layer(x, doc, Wq, Wk, Wv, H, scaling=True, lengths=None, mask=None, g=None):
    """TargetAttentionLayer as defined: Q = doc W_query, K_l = x_l W_key, V_l = x_l W_value per head, masked softmax of <Q_h, K_lh> / sqrt(d),
    out = concat_h sum_l a_hl V_lh.  g (B, E) or None -> dict(out (B, E), dx, ddoc, dWq, dWk, dWv), all fp64."""
    x64, doc64 = np.asarray(x, dtype=np.float64), np.asarray(doc, dtype=np.float64)
    Wq, Wk, Wv = (np.asarray(w, dtype=np.float64) for w in (Wq, Wk, Wv))
    B, L, D = x64.shape
    E = Wq.shape[1]
    d = E // H
    c = 1.0 / math.sqrt(d) if scaling else 1.0
    key = keys_of(B, L, lengths, mask)
    out = np.zeros((B, E))
    dx, ddoc = np.zeros_like(x64), np.zeros_like(doc64)
    dWq, dWk, dWv = np.zeros_like(Wq), np.zeros_like(Wk), np.zeros_like(Wv)
    g64 = None if g is None else np.asarray(g, dtype=np.float64)
    for b in range(B):
        ls = [l for l in range(L) if key[b, l]]
        if not ls:
            continue
        for h in range(H):
            cols = slice(h * d, (h + 1) * d)
            Q = doc64[b] @ Wq[:, cols]
            K = {l: x64[b, l] @ Wk[:, cols] for l in ls}
            V = {l: x64[b, l] @ Wv[:, cols] for l in ls}
            s = {l: c * float(np.dot(Q, K[l])) for l in ls}
            top = max(s.values())
            total = 0.0
            for l in ls:
                total += math.exp(s[l] - top)
            a = {l: math.exp(s[l] - top) / total for l in ls}
            for l in ls:
                out[b, cols] += a[l] * V[l]
            if g64 is None:
                continue
            go = g64[b, cols]
            da = {l: float(np.dot(go, V[l])) for l in ls}
            mean = 0.0
            for l in ls:
                mean += a[l] * da[l]
            dQ = np.zeros(d)
            for l in ls:
                dsl = a[l] * (da[l] - mean)
                dV, dK = a[l] * go, (c * dsl) * Q
                dQ += (c * dsl) * K[l]
                dWv[:, cols] += np.outer(x64[b, l], dV)
                dWk[:, cols] += np.outer(x64[b, l], dK)
                dx[b, l] += Wv[:, cols] @ dV + Wk[:, cols] @ dK
            dWq[:, cols] += np.outer(doc64[b], dQ)
            ddoc[b] += Wq[:, cols] @ dQ
    return dict(out=out, dx=dx, ddoc=ddoc, dWq=dWq, dWk=dWk, dWv=dWv)


# ---- measures ------------------------------------------------------------------------------------------------------------------------

def rowfrac(got, ref, tol=TOL):
    """Worst fraction of the per-row bound tol * max(1, max |ref row|) over the rows (last axis) of got - ref; inf for a NaN or a shape mismatch."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return float('inf')
    if got.size == 0:
        return 0.0
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    err = np.abs(got - ref).max(axis=1)
    bound = tol * np.maximum(1.0, np.abs(ref).max(axis=1))
    f = err / bound
    return float('inf') if np.isnan(f).any() else float(f.max())


def tensorfrac(got, ref, tol=TOL):
    """Fraction of the per-tensor bound tol * max(1, max |ref|) (weight gradients)."""
    return rowfrac(np.asarray(got).reshape(1, -1), np.asarray(ref).reshape(1, -1), tol)


def lsefrac(got, ref):
    """Worst fraction of TOL_LSE * max(1, |lse|); -inf must be met exactly."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if got.shape != ref.shape:
        return float('inf')
    empty = np.isneginf(ref)
    if not np.array_equal(np.isneginf(got), empty):
        return float('inf')
    if empty.all():
        return 0.0
    f = np.abs(got[~empty] - ref[~empty]) / (TOL_LSE * np.maximum(1.0, np.abs(ref[~empty])))
    return float('inf') if np.isnan(f).any() else float(f.max())


# ---- shapes and inputs ---------------------------------------------------------------------------------------------------------------

def shapes(spw, trip, lanes):
    """(B, L, D, H) placed from recnow_attention_softmax_tile: spw samples per wave, trip float4 pieces per loop trip, lanes per sample.
    The vector route takes D = 4 CPL, CPL in {1, 2, 4, 8, 16}: L = trip / CPL positions fill exactly one trip.  B = spw is a full wave,
    spw +- 1 and 2 spw + 1 ragged ones, 1 a wave with one sample.  Every other D takes the guarded route (16 / 32 / 64 lanes per sample)."""
    out = [(1, 1, 1, 1), (3, 15, 3, 2), (spw + 1, 17, 3, 3), (2 * spw + 1, 16, 1, 8)]                     # guarded, 16 lanes
    for cpl, Bs, Hs in ((1, (spw, spw + 1, 3), (1, 3, 2)), (2, (spw + 1, spw, 1), (2, 1, 8)), (4, (3, 2 * spw + 1, spw), (8, 3, 1)),
                        (8, (spw, 1, spw + 1), (2, 8, 3)), (16, (spw + 1, 3, spw), (3, 2, 8))):
        one = trip // cpl
        out += [(Bs[0], one, 4 * cpl, Hs[0]), (Bs[1], one + 1, 4 * cpl, Hs[1]), (Bs[2], 2 * one + 2, 4 * cpl, Hs[2])]
    out += [(spw, 1, 64, 2), (3, 15, 16, 1), (2 * spw + 1, 130, 4, 2), (3, 65, 32, 2), (spw, 64, 64, 1)]   # vector, the issue's L
    out += [(3, 17, 20, 2), (spw + 1, 16, 20, 8), (spw, 64, 30, 1)]                                        # guarded, 32 lanes
    out += [(spw + 1, 16, 65, 3), (3, 17, 256, 8), (spw, 130, 256, 2), (1, 65, 100, 1), (2 * spw + 1, 15, 128, 2)]   # guarded, 64 lanes
    return out


def draw(rng, B, L, D, H, mode):
    """Standard-normal x (B, L, D), q (B, H, D), dc (B, H, D) in fp32; lengths uniform in 0 .. L and / or a mask with 20 % of the positions
    off, as the mode says.  Sample 0 is always full-length, and sample B - 1 (B >= 2) is always empty in every mode that can mask."""
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    q = rng.standard_normal((B, H, D)).astype(np.float32)
    dc = rng.standard_normal((B, H, D)).astype(np.float32)
    lengths = mask = None
    if mode in ('lengths', 'both'):
        lengths = rng.integers(0, L + 1, B).astype(np.int64)
        lengths[0] = L
    if mode in ('mask', 'both'):
        mask = (rng.random((B, L)) >= 0.2).astype(np.uint8)
        mask[0] = 1
    if B >= 2:
        if mode == 'lengths' or (mode == 'both' and B % 2 == 0):
            lengths[B - 1] = 0
        elif mode in ('mask', 'both'):
            mask[B - 1] = 0
    return x, q, dc, lengths, mask


@functools.lru_cache(maxsize=None)
def case(B, L, D, H, mode, seed=0):
    """The inputs of one (shape, mode) and their oracle, computed once and shared; treat as read-only."""
    x, q, dc, lengths, mask = draw(np.random.default_rng([seed, B, L, D, H, MODES.index(mode)]), B, L, D, H, mode)
    ref = run(x, q, lengths, mask, None, dc)
    for v in (x, q, dc, lengths, mask) + tuple(ref.values()):
        if v is not None:
            v.setflags(write=False)
    return dict(x=x, q=q, dc=dc, lengths=lengths, mask=mask, ref=ref)


def large_scores(D, L):
    """Scores of magnitude 100 from exactly representable inputs: B = L samples, q = (+-10, 0, ..) (head 1 negates head 0), x[b, l, 0] = v_l an
    integer in -9 .. 8, scale 1.  Sample b has v = 10 (score 100, the largest of head 0) at position b and v = 9.875 at b + 1; v = -10 and -9.875
    (head 1's largest two) at b + 7 and b + 8, all mod L: the maximum visits every position.  Conditioning of the backward: a weight that sits
    on ONE key makes g - gbar, and with it dx and dquery, cancel to nothing while the fp32 error of the two dot products stays eps |dc| |x|
    times the factor scale |q| = 10 -- the plain fp32 composition misses the row bound by 2x to 4x on such inputs.  So the two largest keys of a
    head share the weight (0.78 / 0.22) and differ as much as they can in the other columns (+-8 along the sign of dc, |dc| >= 0.5): g - gbar
    is then as large as g itself.  -> x (L, L, D), q (L, 2, D), dc (L, 2, D) in fp32."""
    B = L
    rng = np.random.default_rng([31, D, L])
    i = np.arange(B)
    dc = rng.standard_normal((B, 2, D))
    dc = (np.sign(dc) * (0.5 + np.abs(dc))).astype(np.float32)
    x = rng.integers(-8, 9, (B, L, D)).astype(np.float32)
    v = rng.integers(-9, 9, (B, L)).astype(np.float32)
    for pos, val, h, side in (((i + 0) % L, 10.0, 0, 8.0), ((i + 1) % L, 9.875, 0, -8.0), ((i + 7) % L, -10.0, 1, 8.0), ((i + 8) % L, -9.875, 1, -8.0)):
        v[i, pos] = val
        x[i, pos] = side * np.sign(dc[:, h])
    x[:, :, 0] = v
    q = np.zeros((B, 2, D), dtype=np.float32)
    q[:, 0, 0], q[:, 1, 0] = 10.0, -10.0
    return x, q, dc

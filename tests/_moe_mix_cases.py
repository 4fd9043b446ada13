"""Cases, data, the fp64 reference and a plain fp32 restatement of the softmax-gate mixing kernels (csrc/layers.hip recnow_moe_mix_fwd / _bwd:
k_moe_mix_fwd, one wave per (t, b) row, columns in trips of 64; k_moe_mix_bwd, one wave per batch row; both on at most 4096 workgroups of 4 rows).
Used by tests/test_moe_mix_gpu.py (on the GPU) and tests/test_moe_mix_cases_cpu.py (coverage of the cases; the restatement meets the bounds).

A covering subset, not the cross product: every N in {1, 2, 5, 63, 64}, U in {1, 63, 64, 65, 130}, T in {1, 3}, B in {1, 5, 700}, every kind of
logits and every form of the backward appears, each with the forward and with the backward.

Two choices keep `per row against the row's max |ref|` a bound that fp32 arithmetic can meet at all (per ENTRY every result is also held to the sum
of |terms| of that entry, which needs no such care):
  * a row of dexperts with ONE entry (U = 1) is a sum over the T tasks that may cancel: the U = 1 cases have T = 1;
  * a row of dlogits at N = 2 is +- g1 g2 (dg1 - dg2), a difference of two dot products that may cancel: the N = 2 cases with a free second gate
    have 5 rows.  ('spread80' and 'dominant' rows have the gates (1, 0, ..) in fp32: their dlogits are exactly 0 and must come out so.)
tests/test_moe_mix_cases_cpu.py holds the fp32 restatement of EVERY case to half of every bound, on the same data."""
import zlib

import numpy as np

MOE_MAX_N = 64
GRID_ROWS = 4096 * 4              # rows of one trip at the cap of moe_grid

KINDS = ('normal', 'equal', 'spread80', 'dominant', 'offset1e4')
FORMS = ('plain', 'accumulate', 'no_dexperts', 'no_dlogits')

CASES = []


def case(T, B, N, U, kind, form):
    CASES.append(dict(name='t%d_b%d_n%d_u%d_%s_%s' % (T, B, N, U, kind, form), T=T, B=B, N=N, U=U, kind=kind, form=form))


case(3, 700, 5, 63, 'normal', 'plain')
case(1, 5, 1, 1, 'equal', 'accumulate')
case(3, 1, 2, 64, 'spread80', 'no_dexperts')
case(1, 700, 63, 65, 'dominant', 'no_dlogits')
case(3, 5, 64, 130, 'offset1e4', 'accumulate')
case(1, 1, 64, 1, 'normal', 'plain')
case(3, 700, 2, 130, 'spread80', 'plain')
case(1, 5, 5, 64, 'dominant', 'plain')
case(3, 5, 63, 63, 'offset1e4', 'plain')
case(1, 700, 1, 65, 'offset1e4', 'no_dexperts')
case(1, 5, 2, 63, 'normal', 'plain')
case(3, 5, 2, 65, 'equal', 'accumulate')
case(3, 5, 64, 64, 'spread80', 'accumulate')
case(3, GRID_ROWS // 3 + 1, 5, 65, 'normal', 'plain')           # T B = 16 386 rows > 16 384 > B: the forward's grid-stride loop only
case(1, GRID_ROWS + 5, 5, 65, 'normal', 'accumulate')           # B = 16 389: both loops


def make(c):
    """fp32 inputs of a case: logits (T, B, N), experts (N, B, U), dout (T, B, U), prefill (N, B, U) (read with form 'accumulate' only)"""
    T, B, N, U = c['T'], c['B'], c['N'], c['U']
    rng = np.random.default_rng(zlib.crc32(c['name'].encode()))
    lg = rng.standard_normal((T, B, N))
    rows = np.arange(T * B).reshape(T, B)
    if c['kind'] == 'equal':
        lg = np.broadcast_to(rng.standard_normal((T, B, 1)), (T, B, N)).copy()
    elif c['kind'] == 'spread80':            # +80 on one logit of the row, -80 or a little below on all others (N = 1: +80 and -80 by turns): the small
        top = rows % N                       # gates are e^-160, below the fp32 range, and come out as exactly 0
        lg = -80.0 - np.abs(lg)
        if N >= 2:
            np.put_along_axis(lg, ((top + 1) % N)[..., None], -80.0, -1)
            np.put_along_axis(lg, top[..., None], 80.0, -1)
        else:
            lg[...] = np.where(rows % 2 == 1, -80.0, 80.0)[..., None]
    elif c['kind'] == 'dominant':
        np.put_along_axis(lg, (rows % N)[..., None], 1e4, -1)
    elif c['kind'] == 'offset1e4':           # softmax is shift-invariant: the fp64 gates change only through the fp32 rounding of the inputs
        lg = lg + np.where(rows % 2 == 0, 1e4, -1e4)[..., None]
    f = lambda a: a.astype(np.float32)      # noqa: E731
    return dict(logits=f(lg), experts=f(rng.standard_normal((N, B, U))), dout=f(rng.standard_normal((T, B, U))),
                prefill=f(rng.standard_normal((N, B, U))))


def forward64(inp):
    """gates, out, sum of |terms| of out"""
    lg, E = inp['logits'].astype(np.float64), inp['experts'].astype(np.float64)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    g = e / e.sum(-1, keepdims=True)
    return g, np.einsum('tbn,nbu->tbu', g, E), np.einsum('tbn,nbu->tbu', g, np.abs(E))


def backward64(c, inp, gates32):
    """fp64 backward of the fp32 inputs (the gates are an input of the backward).  {name: (ref, sum of |terms|)} of dexperts (N, B, U), dlogits (T, B, N)"""
    g, E, do = gates32.astype(np.float64), inp['experts'].astype(np.float64), inp['dout'].astype(np.float64)
    de, mde = np.einsum('tbn,tbu->nbu', g, do), np.einsum('tbn,tbu->nbu', g, np.abs(do))
    if c['form'] == 'accumulate':
        de, mde = de + inp['prefill'], mde + np.abs(inp['prefill'])
    dg, mdg = np.einsum('tbu,nbu->tbn', do, E), np.einsum('tbu,nbu->tbn', np.abs(do), np.abs(E))
    dl = g * (dg - (g * dg).sum(-1, keepdims=True))
    mdl = g * (mdg + (g * mdg).sum(-1, keepdims=True))
    return dict(dexperts=(de, mde), dlogits=(dl, mdl))


def forward32(inp):
    """the same formulas in plain fp32, sums taken in order"""
    lg, E = inp['logits'], inp['experts']
    e = np.exp(lg - lg.max(-1, keepdims=True), dtype=np.float32)
    s = np.zeros(lg.shape[:2], np.float32)
    for n in range(lg.shape[2]):
        s = s + e[..., n]
    g = e / s[..., None]
    out = np.zeros(lg.shape[:2] + (E.shape[2],), np.float32)
    for n in range(lg.shape[2]):
        out = out + g[..., n, None] * E[n][None]
    return g, out


def backward32(c, inp, g):
    E, do = inp['experts'], inp['dout']
    T, B, N = g.shape
    de = np.zeros(E.shape, np.float32)
    for t in range(T):
        de = de + g[t].T[:, :, None] * do[t][None]
    if c['form'] == 'accumulate':
        de = inp['prefill'] + de
    dg = np.zeros((T, B, N), np.float32)
    for u in range(E.shape[2]):
        dg = dg + do[:, :, u, None] * E[:, :, u].T[None]
    dot = np.zeros((T, B), np.float32)
    for n in range(N):
        dot = dot + g[..., n] * dg[..., n]
    return dict(dexperts=de, dlogits=g * (dg - dot[..., None]))


def margins(ref, mag, got, rel):
    """(worst |err| / (rel sum of |terms|) over the entries, worst |err| / (rel max |ref| of the row) over the rows); a row whose reference is all
    zero must be matched exactly (fraction 0 or inf)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = np.where(err == 0, 0.0, err / (rel * mag))
        row = np.where(err.max(-1) == 0, 0.0, err.max(-1) / (rel * np.abs(ref).max(-1)))
    return float(ent.max()), float(row.max())

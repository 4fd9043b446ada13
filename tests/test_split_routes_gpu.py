"""Every split-precision product route, term by term against fp64 (tests/_split_census.py), in both arithmetics.

Long-K products (rn_gemm_launch_split, csrc/gemm_split.hip).  A product reaches the split launcher when `split_ok` holds (csrc/gemm.hip
rn_gemm_impl: precision 1, a side product (sp_r > 0), lean 128 x 128 tiles, K > 256, a_mode NONE or MUL; A [M][K] with B [K][N] only without
a_mode); it gets B split into planes when `split_planes_shape` holds (csrc/gemm.hip: N = 128, batch 1, A [M][K] with K <= 4096, or A [K][M]
x B [K][N] under RECNOW_SPLIT_LEAN=2); the lean kernel k_gemm_s3 takes it when `s3_shape` holds (sp_r <= 2, whole chunks of 32 k, chunk <= 2048);
`s3_launch` picks the PAIR form for k-contiguous A rows that start on a 128-byte line (lda % 32 == 0, chunks of 64 k, RECNOW_S3_PAIR != 0).
Everything else runs k_gemm_split, with planes (A [M][K], K <= 4096) or without.  The switches are read once per process: every
environment below runs in a child process of its own.

Each row checks, in precision 1 and (same inputs) precision 0:
  1. the census inputs give exactly the expected bits for C and the side product;
  2. on random data, precision 1 is not bit-identical to precision 0 (the split kernel ran; no silent fall-back);
  3. the fp64 bound on random data, max |C - R| <= 1e-5 max |R|, and per element |C - R|_ij <= C_ELEM (|A'||B|)_ij, side product included;
  4. non-finite operands stay where they belong: an output whose fp64 reference is non-finite is non-finite, every other output (side product
     included) is bit-identical to the clean run;
  5. operands at the top of the fp32 range (3.3961e38 <= |x| <= FLT_MAX, where bf16 rounding gives inf) give finite results within the bound.
The step-size rows (M = 65 536 x K = 1024, K = 65 536 split over K) run 2 and 3 only, one per kernel family: their census operands would take
gigabytes on the host.

Short-K products (K = 144, rn_gemm_launch_shortk_split / rn_gemm_launch_shortk, csrc/gemm_shortk.hip): every form the split launcher accepts,
with the workspace of recnow_gemm_workspace_bytes, in both arithmetics, with checks 1-5 (1 and 4 on 256 x 256, 2, 3 and 5 also on the
ragged 8576 x 1024), once more with k_valid = 130 and zero padding."""
import ctypes
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# per-element bound on random data, |C - R|_ij <= C_ELEM (|A'||B|)_ij: a host emulation of the six-term product with fp32 accumulation per
# 16-k MFMA step gave at most 1.7e-7 (K = 144), 1.4e-7 (K = 1024, the N(0, 0.05^2) operands included), 1.1e-7 (K = 8192); 1e-6 is 6x that
C_ELEM = 1e-6
BF16_TOP = 3.3961e38                       # the smallest fp32 magnitude that bf16 round-to-nearest-even takes to inf
FLT_MAX = float(np.finfo(np.float32).max)

# ---- the long-K route table ----------------------------------------------------------------------------------------------------------------
# (name, env, instantiation reached, ta, tb, mul, M, K, extra) -- extra: sp_r (default 2), off (A starts `off` floats into a 128-byte line),
# perm (c_perm_s), step (step-size row: random checks only, operands N(0, scale^2))
ROUTES = [
    ('s3_pair_gemm1', '', 'k_gemm_s3<true,0,PAIR>', 0, 0, 0, 1024, 1024, {}),
    ('s3_pair_dt2g', '', 'k_gemm_s3<true,0,PAIR>', 0, 1, 0, 1024, 1024, {}),
    ('s3_pair_dt2g_mul', '', 'k_gemm_s3<true,MUL,PAIR>', 0, 1, 1, 1024, 1024, {}),
    ('s3_twoset_off_gemm1', '', 'k_gemm_s3<true,0>', 0, 0, 0, 1024, 1024, {'off': 16}),
    ('s3_twoset_off_dt2g_mul', '', 'k_gemm_s3<true,MUL>', 0, 1, 1, 1024, 1024, {'off': 16}),
    ('split_planes_sp3', '', 'k_gemm_split<true,0,2>', 0, 0, 0, 1024, 1024, {'sp_r': 3}),
    ('split_planes_sp4_mul', '', 'k_gemm_split<true,1,2>', 0, 1, 1, 1024, 1024, {'sp_r': 4}),
    ('split_gemm1_k8192', '', 'k_gemm_split<true,0,0>', 0, 0, 0, 256, 8192, {}),
    ('split_dt2g_k8192', '', 'k_gemm_split<true,0,1>', 0, 1, 0, 256, 8192, {}),
    ('split_dt2g_mul_k8192', '', 'k_gemm_split<true,1,1>', 0, 1, 1, 256, 8192, {}),
    ('split_du', '', 'k_gemm_split<false,0,0>', 1, 0, 0, 1024, 8192, {}),
    ('split_dwt_mul', '', 'k_gemm_split<false,1,0>', 1, 0, 1, 1024, 8192, {}),
    ('split_du_cperm', '', 'k_gemm_split<false,0,0> c_perm_s', 1, 0, 0, 1024, 8192, {'perm': 64}),
    ('s3_pair_step', '', 'k_gemm_s3<true,MUL,PAIR>', 0, 1, 1, 65536, 1024, {'step': 0.05}),
    ('split_du_step', '', 'k_gemm_split<false,0,0>', 1, 0, 0, 1024, 65536, {'step': 0.05}),
    ('s3_twoset_gemm1', 'RECNOW_S3_PAIR=0', 'k_gemm_s3<true,0>', 0, 0, 0, 1024, 1024, {}),
    ('s3_twoset_dt2g_mul', 'RECNOW_S3_PAIR=0', 'k_gemm_s3<true,MUL>', 0, 1, 1, 1024, 1024, {}),
    ('s3_krow_du', 'RECNOW_SPLIT_LEAN=2', 'k_gemm_s3<false,0>', 1, 0, 0, 1024, 8192, {}),
    ('s3_krow_dwt_mul', 'RECNOW_SPLIT_LEAN=2', 'k_gemm_s3<false,MUL>', 1, 0, 1, 1024, 8192, {}),
    ('lean0_gemm1', 'RECNOW_SPLIT_LEAN=0', 'k_gemm_split<true,0,2>', 0, 0, 0, 1024, 1024, {}),
    ('lean0_dt2g_mul', 'RECNOW_SPLIT_LEAN=0', 'k_gemm_split<true,1,2>', 0, 1, 1, 1024, 1024, {}),
    ('lean0_gemm1_step', 'RECNOW_SPLIT_LEAN=0', 'k_gemm_split<true,0,2>', 0, 0, 0, 65536, 1024, {'step': 0.05}),
]
ENVS = sorted({r[1] for r in ROUTES})

# ---- the short-K forms (K = 144): (name, b_trans, ep (bit 0: emul, bit 1: accumulate), c2_mode) ------------------------------------------
SHORTK = [('fwd_c0', 0, 1, 0), ('fwd_c1', 0, 1, 1), ('fwd_c3_head', 0, 1, 3), ('fwd0', 0, 0, 0), ('acc_bnk', 1, 2, 0), ('bnk_c0', 1, 0, 0),
          ('bnk_c2', 1, 0, 2), ('bnk_c4', 1, 0, 4), ('bnk_c5', 1, 0, 5), ('bnk_c6', 1, 0, 6)]


def _set_precision(mode):
    from rec_now_amd import _lib
    _lib.call('recnow_set_gemm_precision', mode)
    assert _lib.load().recnow_get_gemm_precision() == mode


def _gemm(d, dev):
    from rec_now_amd import _lib
    lib = _lib.load()
    ws = _lib.workspace(lib.recnow_gemm_workspace_bytes(ctypes.byref(d)), dev)
    _lib.call('recnow_gemm', ctypes.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream())
    torch.cuda.synchronize()


def run_longk(dev, ta, tb, A, A2, B, Bx, off=0, perm=0):
    """C = op(A [* A2]) op(B), Cx = op(A [* A2]) Bx through recnow_gemm.  A, A2: logical (M, K); B: (K, N); Bx: (K, sp_r).  Returns C (M, N), Cx."""
    from rec_now_amd import _lib
    M, K = A.shape
    N, R = B.shape[1], Bx.shape[1]

    def store(x):      # the stored layout of A (a_trans), `off` floats into a row of lda = K + 32
        if ta:
            return torch.from_numpy(np.ascontiguousarray(x.T)).to(dev), M
        if off:
            w = np.zeros((M, K + 32), np.float32)
            w[:, off:off + K] = x
            return torch.from_numpy(w).to(dev), K + 32
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev), K
    Ad, lda = store(A)
    A2d = store(A2)[0] if A2 is not None else None
    Bd = torch.from_numpy(np.ascontiguousarray(B.T if tb else B)).to(dev)
    Bxd = torch.from_numpy(np.ascontiguousarray(Bx)).to(dev)
    C = torch.full((M * N,), 7.0, device=dev)
    Cx = torch.full((M, R), 7.0, device=dev)
    d = _lib.GemmDesc()
    d.A, d.lda, d.a_trans = Ad.data_ptr() + 4 * off, lda, ta
    if A2 is not None:
        d.A2, d.a_mode = A2d.data_ptr() + 4 * off, 1
    d.B, d.ldb, d.b_trans = Bd.data_ptr(), (K if tb else N), tb
    d.C, d.ldc = C.data_ptr(), N
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.c_perm_s = perm
    d.sp_bx, d.sp_cx, d.sp_bx_ks, d.sp_bx_rs, d.sp_cx_ms, d.sp_cx_rs, d.sp_r = Bxd.data_ptr(), Cx.data_ptr(), R, 1, R, 1, R
    _gemm(d, dev)
    C = C.cpu().numpy()
    C = C.reshape(N // perm, M, perm).transpose(1, 0, 2).reshape(M, N) if perm else C.reshape(M, N)
    return C, Cx.cpu().numpy()


def _ref(A, A2, B, Bx):
    Ap = A.astype(np.float64) * (A2.astype(np.float64) if A2 is not None else 1.0)
    B64 = B.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return Ap @ B64, Ap @ Bx.astype(np.float64), np.abs(Ap) @ np.abs(B64), np.abs(Ap) @ np.abs(Bx.astype(np.float64))


def _bound(tag, got, R, den):
    err = np.abs(got - R)
    assert np.isfinite(got).all(), '%s: non-finite output' % tag
    assert err.max() <= 1e-5 * np.abs(R).max(), '%s: max err %.3g vs max|R| %.3g' % (tag, err.max(), np.abs(R).max())
    ratio = (err / np.maximum(den, 1e-300)).max()
    assert ratio <= C_ELEM, '%s: per-element err / (|A||B|) = %.3g > %.3g' % (tag, ratio, C_ELEM)


def _nonfinite(tag, got, clean, R):
    bad = ~np.isfinite(R)
    assert bad.any()
    assert not np.isfinite(got[bad]).any(), '%s: %d outputs with a non-finite reference are finite' % (tag, int(np.isfinite(got[bad]).sum()))
    assert np.array_equal(got[~bad], clean[~bad]), '%s: %d finite outputs differ from the clean run' % (tag, int((got[~bad] != clean[~bad]).sum()))


def _poison(rng, M, K, N, R, kslab=None):
    """(A row, k, value) / (k, B column, value) / (k, side column, value) plants: +inf, -inf and NaN in single elements."""
    ks = rng.choice(K if kslab is None else kslab, 4, replace=False)
    rows = rng.choice(M, 2, replace=False)
    return [('A', rows[0], ks[0], np.inf), ('A', rows[1], ks[1], -np.inf), ('B', ks[2], int(rng.integers(N)), np.nan),
            ('Bx', ks[3], int(rng.integers(R)), np.nan)]


def check_longk_route(dev, name, ta, tb, mul, M, K, extra):
    N, R, off, perm, step = 128, extra.get('sp_r', 2), extra.get('off', 0), extra.get('perm', 0), extra.get('step')
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    run = lambda A, A2, B, Bx: run_longk(dev, ta, tb, A, A2, B, Bx, off=off, perm=perm)      # noqa: E731
    scale = step if step else 1.0
    A = (rng.standard_normal((M, K)) * scale).astype(np.float32)
    A2 = rng.uniform(-1, 1, (M, K)).astype(np.float32) if mul else None
    B = (rng.standard_normal((K, N)) * scale).astype(np.float32)
    Bx = rng.standard_normal((K, R)).astype(np.float32)
    Rc, Rx, den, denx = _ref(A, A2, B, Bx)
    out = {}
    for prec in (0, 1):
        _set_precision(prec)
        out[prec] = run(A, A2, B, Bx)
        _bound('%s p%d C' % (name, prec), out[prec][0], Rc, den)
        _bound('%s p%d Cx' % (name, prec), out[prec][1], Rx, denx)
    assert not np.array_equal(out[0][0], out[1][0]), '%s: precision 1 is bit-identical to precision 0: the split kernel did not run' % name
    if step:
        return
    from _split_census import make
    for case in ('d',) if mul else ('a', 'b', 'c'):
        c = make(M, N, K, case=case, seed=len(name), sp_r=R)
        for prec in (0, 1):
            _set_precision(prec)
            C, Cx = run(c.A, c.A2, c.B, c.Bx)
            wrong = np.flatnonzero(C != c.C)
            assert wrong.size == 0, '%s p%d census %s: %d outputs wrong, first (%d, %d): %r vs %r' % (
                name, prec, case, wrong.size, wrong[0] // N, wrong[0] % N, C.flat[wrong[0]], c.C.flat[wrong[0]])
            assert np.array_equal(Cx, c.Cx), '%s p%d census %s: side product wrong in %d rows' % (name, prec, case, int((Cx != c.Cx).any(1).sum()))
    # non-finite plants (one k-slab: the first 256 k, a chunk of its own whenever the product is split over K)
    Ap, Bp, Bxp = A.copy(), B.copy(), Bx.copy()
    for what, i, j, v in _poison(rng, M, K, N, R, kslab=256):
        {'A': Ap, 'B': Bp, 'Bx': Bxp}[what][i, j] = v
    Rn, Rxn = _ref(Ap, A2, Bp, Bxp)[:2]
    for prec in (0, 1):
        _set_precision(prec)
        C, Cx = run(Ap, A2, Bp, Bxp)
        _nonfinite('%s p%d C' % (name, prec), C, out[prec][0], Rn)
        _nonfinite('%s p%d Cx' % (name, prec), Cx, out[prec][1], Rxn)
    # the top of the fp32 range, B scaled so that every product and sum stays finite
    At = (np.sign(A) * rng.uniform(BF16_TOP, FLT_MAX, A.shape)).astype(np.float32)
    At2 = np.sign(A2).astype(np.float32) if mul else None
    Bt, Bxt = (B * 2.0 ** -16 / K).astype(np.float32), (Bx * 2.0 ** -16 / K).astype(np.float32)
    Rt, Rxt, dent, denxt = _ref(At, At2, Bt, Bxt)
    for prec in (0, 1):
        _set_precision(prec)
        C, Cx = run(At, At2, Bt, Bxt)
        _bound('%s p%d top-of-range C' % (name, prec), C, Rt, dent)
        _bound('%s p%d top-of-range Cx' % (name, prec), Cx, Rxt, denxt)


def run_shortk(dev, form, A, B, T, k_valid=0):
    """One short-K product (K = 144, A [M][K]) in form `form` = (name, b_trans, ep, c2_mode).  T: dict of the epilogue tensors (E, C0, D0, E2..E6
    (M, N); rv (M,), cv, hv (N,)).  Returns (C, C2, hp) as numpy (None where the form has no such output)."""
    from rec_now_amd import _lib
    _, tb, ep, c2 = form
    M, K = A.shape
    N = B.shape[1]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in T.items()}
    Ad = torch.from_numpy(A).to(dev)
    Bd = torch.from_numpy(np.ascontiguousarray(B.T if tb else B)).to(dev)
    C = t['C0'].clone() if ep & 2 else torch.full((M, N), 7.0, device=dev)
    C2 = t['D0'].clone()
    hp = torch.full((M, N // 64), 7.0, device=dev)
    d = _lib.GemmDesc()
    d.A, d.lda = Ad.data_ptr(), K
    d.B, d.ldb, d.b_trans = Bd.data_ptr(), (K if tb else N), tb
    d.C, d.ldc = C.data_ptr(), N
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.k_valid = k_valid
    if ep & 1:
        d.emul, d.lde, d.e_mode = t['E'].data_ptr(), N, 1
    d.accumulate = 1 if ep & 2 else 0
    d.c2_mode = c2
    if c2 in (1, 2, 3, 4):
        d.C2, d.ldc2 = C2.data_ptr(), N
    if c2 in (2, 4, 5, 6):
        d.E2, d.lde2 = t['E2'].data_ptr(), N
    if c2 in (4, 5, 6):
        d.E3, d.lde3, d.rv, d.cv = t['E3'].data_ptr(), N, t['rv'].data_ptr(), t['cv'].data_ptr()
    if c2 in (5, 6):
        d.E6 = t['E6'].data_ptr()
    if c2 == 5:
        d.E4, d.E5 = t['E4'].data_ptr(), t['E5'].data_ptr()
    if c2 == 3:
        d.hv, d.hp, d.hp_ld = t['hv'].data_ptr(), hp.data_ptr(), N // 64
    _gemm(d, dev)
    return (None if c2 == 3 else C.cpu().numpy(), C2.cpu().numpy() if c2 in (1, 2, 3, 4) else None, hp.cpu().numpy() if c2 == 3 else None)


def shortk_ref(form, A, B, T):
    """fp64 reference of each form (include/recnow.h, recnow_gemm_desc), with the per-element error scales: returns [(C, C2, hp), (dC, dC2, dhp)]
    where d* = C_ELEM |A||B| carried through the epilogue plus 2^-22 of the other terms' magnitudes."""
    _, tb, ep, c2 = form
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    g = {k: v.astype(np.float64) for k, v in T.items()}
    with np.errstate(invalid='ignore', over='ignore'):
        P, den = A64 @ B64, C_ELEM * (np.abs(A64) @ np.abs(B64))
        u = 2.0 ** -22
        C, dC = P, den
        C2 = dC2 = hp = dhp = None
        if ep & 1:
            C, dC = P * g['E'], den * np.abs(g['E']) + u * np.abs(P * g['E'])
        if ep & 2:
            C, dC = C + g['C0'], dC + u * (np.abs(C) + np.abs(g['C0']))
        if c2 == 1 or c2 == 3:
            C2, dC2 = P, den
        if c2 == 2:
            C2, dC2 = g['D0'] + P * g['E2'], den * np.abs(g['E2']) + u * (np.abs(g['D0']) + np.abs(P * g['E2']))
        rc = g['rv'][:, None] * g['cv'][None, :] if c2 >= 4 else None
        if c2 == 4:
            extra = rc * g['E3']
            C2, dC2 = P * g['E2'] + extra, den * np.abs(g['E2']) + u * (np.abs(P * g['E2']) + np.abs(extra))
        if c2 in (5, 6):
            ex = g['E2'] * g['E3'] + rc * g['E6'] + (g['E4'] * g['E5'] if c2 == 5 else 0.0)
            mag = np.abs(g['E2'] * g['E3']) + np.abs(rc * g['E6']) + (np.abs(g['E4'] * g['E5']) if c2 == 5 else 0.0)
            C, dC = P + ex, den + u * (np.abs(P) + mag)
        if c2 == 3:
            M, N = P.shape
            Y = (P * g['E'] * g['hv'][None, :]).reshape(M, N // 64, 64)
            hp = Y.sum(2)
            dhp = ((den * np.abs(g['E']) * np.abs(g['hv'])[None, :]).reshape(M, N // 64, 64).sum(2) + u * np.abs(Y).sum(2))
            C, dC = None, None
    return (C, C2, hp), (dC, dC2, dhp)


def _shortk_tensors(rng, M, N, exact=False):
    """Epilogue tensors: random, or (census) powers of two for the multipliers and zeros for the added terms, so that the exact product stays exact."""
    if exact:
        p2 = lambda *s: np.ldexp(rng.choice([-1.0, 1.0], s), rng.integers(-1, 2, s)).astype(np.float32)      # noqa: E731
        z = np.zeros((M, N), np.float32)
        return dict(E=p2(M, N), C0=z, D0=z, E2=p2(M, N), E3=z, E4=z, E5=z, E6=z, rv=np.zeros(M, np.float32), cv=np.zeros(N, np.float32),
                    hv=p2(N))
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)      # noqa: E731
    return dict(E=u(M, N), C0=u(M, N), D0=u(M, N), E2=u(M, N), E3=u(M, N), E4=u(M, N), E5=u(M, N), E6=u(M, N), rv=u(M), cv=u(N), hv=u(N))


def _shortk_bound(tag, got, ref):
    (refs, dens) = ref
    for g, r, dd, what in zip(got, refs, dens, ('C', 'C2', 'hp')):
        if r is None:
            continue
        assert np.isfinite(g).all(), '%s %s: non-finite output' % (tag, what)
        err = np.abs(g - r)
        assert (err <= dd + 1e-30).all(), '%s %s: %d elements beyond the bound, worst err %.3g' % (tag, what, int((err > dd).sum()), err.max())


def check_shortk_form(dev, form):
    name, tb, ep, c2 = form
    K = 144
    for M, N in ((256, 256), (8576, 1024)):
        for kv in (0, 130):
            rng = np.random.default_rng(M + kv + 17 * c2 + 3 * ep + tb)
            A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
            B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
            if kv:
                A[:, kv:] = 0
                B[kv:] = 0
            T = _shortk_tensors(rng, M, N)
            ref = shortk_ref(form, A, B, T)
            tag = '%s %dx%d k_valid=%d' % (name, M, N, kv)
            out = {}
            for prec in (0, 1):
                _set_precision(prec)
                out[prec] = run_shortk(dev, form, A, B, T, kv)
                _shortk_bound('%s p%d' % (tag, prec), out[prec], ref)
            first = next(i for i in range(3) if out[0][i] is not None)
            assert not np.array_equal(out[0][first], out[1][first]), '%s: precision 1 is bit-identical to precision 0' % tag
            # top of the fp32 range
            At = (np.sign(A) * rng.uniform(BF16_TOP, FLT_MAX, A.shape)).astype(np.float32)
            Bt = (B * 2.0 ** -16 / K).astype(np.float32)
            reft = shortk_ref(form, At, Bt, T)
            for prec in (0, 1):
                _set_precision(prec)
                _shortk_bound('%s p%d top-of-range' % (tag, prec), run_shortk(dev, form, At, Bt, T, kv), reft)
            if M != 256:
                continue
            from _split_census import make
            for case in 'abc':
                c = make(M, N, K, case=case, seed=M + c2, sp_r=0, k_valid=kv or None)
                Te = _shortk_tensors(rng, M, N, exact=True)
                (eC, eC2, _), _ = shortk_ref(form, c.A, c.B, Te)
                for prec in (0, 1):
                    _set_precision(prec)
                    C, C2, _ = run_shortk(dev, form, c.A, c.B, Te, kv)
                    if eC is not None:
                        assert np.array_equal(C, eC), '%s p%d census %s: %d outputs of C wrong' % (tag, prec, case, int((C != eC).sum()))
                    if eC2 is not None:
                        assert np.array_equal(C2, eC2), '%s p%d census %s: %d outputs of C2 wrong' % (tag, prec, case, int((C2 != eC2).sum()))
            # non-finite plants: +inf / -inf in two A rows, NaN in a B column (below k_valid)
            Ap, Bp = A.copy(), B.copy()
            ks = rng.choice(kv or K, 3, replace=False)
            Ap[3, ks[0]], Ap[130, ks[1]], Bp[ks[2], 77] = np.inf, -np.inf, np.nan
            refn = shortk_ref(form, Ap, Bp, T)[0]
            for prec in (0, 1):
                _set_precision(prec)
                got = run_shortk(dev, form, Ap, Bp, T, kv)
                for g, cl, r, what in zip(got, out[prec], refn, ('C', 'C2', 'hp')):
                    if r is not None:
                        _nonfinite('%s p%d %s' % (tag, prec, what), g, cl, r)


def run_group(env):
    """Child-process entry: every route of one environment, and (default environment) every short-K form.  Prints one JSON line."""
    dev = torch.device('cuda:0')
    res = {}
    jobs = [(r[0], lambda r=r: check_longk_route(dev, r[0], *r[3:])) for r in ROUTES if r[1] == env]
    if env == '':
        jobs += [('shortk_' + f[0], lambda f=f: check_shortk_form(dev, f)) for f in SHORTK]
    for name, job in jobs:
        try:
            job()
            res[name] = 'ok'
        except AssertionError as e:
            res[name] = 'FAIL: %s' % str(e)[:600]
    _set_precision(0)
    print('RESULT ' + json.dumps(res), flush=True)


_SNIPPET = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_split_routes_gpu import run_group
run_group(%r)
'''


@pytest.mark.parametrize('env', ENVS, ids=[e or 'default' for e in ENVS])
def test_split_routes(env):
    """One child process per environment (the switches are read once per process); a child that exits non-zero fails the test, and is not
    retried."""
    extra = dict([env.split('=')]) if env else {}
    r = subprocess.run([sys.executable, '-c', _SNIPPET % (ROOT, os.path.join(ROOT, 'tests'), env)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **extra), cwd=ROOT)
    assert r.returncode == 0, 'child exit %d\n%s\n%s' % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])
    names = [x[0] for x in ROUTES if x[1] == env] + (['shortk_' + f[0] for f in SHORTK] if env == '' else [])
    assert sorted(res) == sorted(names)
    failed = {k: v for k, v in res.items() if v != 'ok'}
    assert not failed, json.dumps(failed, indent=1)

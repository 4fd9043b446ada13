"""Planted-piece census of the split-precision products (rec_now_amd/csrc/gemm_split.hpp `spl_split2`: an fp32 x is split into three bf16
pieces x = x1 + x2 + x3, each round-to-nearest-even, and a product a b is formed as the six bf16 MFMA terms a1b1 a1b2 a2b1 a1b3 a3b1 a2b2 summed
in fp32).

Random operands cannot tell that arithmetic from a weaker one: dropping a3b1 moves the error against fp64 by a few fp32 roundings only.  The
census plants the pieces instead.  Every operand element is p1 + p2 + p3 with small significands (a few bits each) placed so that the host's
round-to-nearest-even decomposition returns exactly the planted pieces, and the three dropped terms a2b3, a3b2, a3b3 are zero.  The nonzero k of
an output are sparse and sit in one exponent window of 24 bits: every partial sum of every term, in any order, is an exact fp32 number.  The
correct six-term kernel (and the exact fp32 kernel) then returns the fp64 product to the bit, whatever its accumulation order; a kernel that
drops, doubles or mispairs a term, reads a stale or wrong piece plane, or loses a k-tile does not.

Sub-cases (`case`):
  'a'  A with three pieces, B exact in bf16 (+-2^f, +-2^(f+1))
  'b'  the reverse
  'c'  both with two pieces (exercises a2b2)
  'd'  A' = A * A2 with A2 in {+-1, +-2, +-1/2} (a_mode MUL: fl32(A A2) is exact before the split), A' planted as in 'a'

Structure: rows fall into row classes (i mod 256 // 8, or i mod 128 // 16 for short K), columns into 16 column classes (j mod 128 // 8), and every
(row class, column class) pair owns `T` k positions: output (i, j) has exactly T nonzero terms, every position of a 128 x 128 tile is covered, and
the used k positions are spread over the whole depth (both halves of a 16-k tile, both k-tiles of a PAIR couple, the first and last k-tile of a
chunk or split-K slab).  Side weights are in {0, +-1}, nonzero at the k of one column class per side column.
"""
import numpy as np
import torch

TERMS = ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2))      # the six terms of the split kernels, (piece of A, piece of B)
WINDOW_BITS = 24                                               # fp32 significand


def bf16_split(x):
    """Host restatement of spl_split2: three round-to-nearest-even bf16 pieces of fp32 `x` (piece 1 from x clamped to +-bf16_max).
    Returns float32 arrays (p1, p2, p3)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    bmax = float(torch.finfo(torch.bfloat16).max)
    p1 = x.clamp(-bmax, bmax).to(torch.bfloat16).float()
    r = x - p1
    p2 = r.to(torch.bfloat16).float()
    r = r - p2
    p3 = r.to(torch.bfloat16).float()
    return p1.numpy(), p2.numpy(), p3.numpy()


def _signs(rng, shape):
    return rng.choice(np.array([-1, 1], dtype=np.int64), shape)


def _planted_ints(rng, shape, npieces, hi):
    """Integer significands of planted values, in units of 2^(e - L) for an element of exponent e:
    three pieces: p1 = s1 2^e (s1 in +-4..5, or +-6..7 where `hi`: the T terms of an output never cancel), p2 = s2 2^(e-10) (+-4..7), p3 = s3 2^(e-19) (+-1..3); L = 19
      |p2 + p3| < 2^(e-7) = half a bf16 spacing below 4 * 2^e, |p3| < 2^(e-17) = half a spacing below 4 * 2^(e-10)
    two pieces:   p1 = s1 2^e (s1 in +-4..5), p2 = s2 2^(e-9) (+-1..3); L = 9 (|p2| <= 0.75 2^(e-7))
    one piece:    +-2^e (+-2^(e+1) where `hi`); L = 0.
    Returns (pieces [3][shape] int64, L)."""
    z = np.zeros(shape, np.int64)
    if npieces == 3:
        return np.stack([_signs(rng, shape) * (rng.integers(4, 6, shape) + 2 * hi) << 19, _signs(rng, shape) * rng.integers(4, 8, shape) << 9,
                         _signs(rng, shape) * rng.integers(1, 4, shape)]), 19
    if npieces == 2:
        return np.stack([_signs(rng, shape) * rng.integers(4, 6, shape) << 9, _signs(rng, shape) * rng.integers(1, 4, shape), z]), 9
    return np.stack([_signs(rng, shape) * (1 + hi), z, z]), 0


class Census:
    """Inputs and exact outputs of one product C = A' B (M x N, depth K), Cx = A' Bx (M x R).
    A, A2, B, Bx: float32, logical layouts (M, K), (M, K) or None, (K, N), (K, R).  C, Cx: float64, exact.
    a, b: float64 pieces [3] of A' (M, K) and B (K, N) -- what spl_split2 must return for them."""


def make(M, N, K, case='a', seed=0, sp_r=2, k_valid=None, T=None):
    """A census of the product of logical shape (M, K) x (K, N).  `k_valid`: the used k all lie below it (a depth padded with zeros).
    T = nonzero terms per output (default: 2 where the depth allows it and the window holds, else 1)."""
    assert case in 'abcd' and N % 8 == 0
    rng = np.random.default_rng(seed)
    kv = K if k_valid is None else k_valid
    nr, rg = (32, 8) if kv >= 512 else (8, 16)                 # row classes, rows per class (period nr * rg)
    nc = 16                                                    # column classes of 8 columns, period 128
    if T is None:
        T = 2 if (kv >= 2 * nr * nc and case != 'c') else 1
    need = nr * nc * T
    assert kv >= need, 'depth %d holds fewer than %d census positions' % (kv, need)
    pos = np.round(np.linspace(0, kv - 1, need)).astype(np.int64).reshape(nr, nc, T)
    assert len(np.unique(pos)) == need
    rc = (np.arange(M) % (nr * rg)) // rg
    cc = (np.arange(N) % 128) // 8
    kr = np.full(K, -1)                                        # row class / column class owning k (-1: unused)
    kc = np.full(K, -1)
    kr[pos.reshape(-1)] = np.repeat(np.arange(nr), nc * T)
    kc[pos.reshape(-1)] = np.tile(np.repeat(np.arange(nc), T), nr)
    amask = kr[None, :] == rc[:, None]                         # (M, K)
    bmask = kc[:, None] == cc[None, :]                         # (K, N)
    npa, npb = {'a': (3, 1), 'b': (1, 3), 'c': (2, 2), 'd': (3, 1)}[case]
    kt = np.zeros(K, np.int64)                                 # term index t of k
    kt[pos.reshape(-1)] = np.tile(np.arange(T), nr * nc)
    ai, La = _planted_ints(rng, (M, K), npa, kt[None, :])
    bi, Lb = _planted_ints(rng, (K, N), npb, kt[:, None])
    ai *= amask
    bi *= bmask
    e = rng.integers(-10, 11, (M, 1))                          # exponent per row of A' and per column of B: the window of output (i, j)
    f = rng.integers(-10, 11, (1, N))                          #   is 2^(e_i + f_j - La - Lb) .. 2^(e_i + f_j - La - Lb + 24)
    # exactness, on Python integers: every term of an output is an integer multiple of its window's unit, and the sum of the absolute values
    # of all its terms stays below 2^24 units -- so every partial sum, in any order, is an fp32 number
    amax = int(np.abs(ai).sum(axis=0).max())                   # sum over pieces of |piece|, worst element
    bmax = int(np.abs(bi).sum(axis=0).max())
    assert T * amax * bmax < 1 << WINDOW_BITS, (T, amax, bmax)
    a = np.ldexp(ai.astype(np.float64), (e - La)[None])
    b = np.ldexp(bi.astype(np.float64), (f - Lb)[None])
    Ap, Bm = a.sum(0), b.sum(0)
    assert np.array_equal(Ap.astype(np.float32).astype(np.float64), Ap) and np.array_equal(Bm.astype(np.float32).astype(np.float64), Bm)
    for full, pieces in ((Ap, a), (Bm, b)):                    # the host decomposition (round to nearest even) returns the planted pieces
        got = bf16_split(full.astype(np.float32))
        for s in range(3):
            assert np.array_equal(got[s].astype(np.float64), pieces[s]), 'piece %d not recovered' % (s + 1)
    c = Census()
    c.case, c.T, c.pos, c.a, c.b = case, T, pos, a, b
    if case == 'd':
        A2 = np.ldexp(_signs(rng, (M, K)).astype(np.float64), rng.integers(-1, 2, (M, K)))      # +-1/2, +-1, +-2
        c.A, c.A2 = (Ap / A2).astype(np.float32), A2.astype(np.float32)
        assert np.array_equal(c.A.astype(np.float64) * A2, Ap)
    else:
        c.A, c.A2 = Ap.astype(np.float32), None
    c.B = Bm.astype(np.float32)
    # side weights: column r sees the k of column class r * (nc - 1) (the first and the last class): T terms of one row's window each
    Bx = np.zeros((K, max(sp_r, 1)), np.float32)
    for r in range(sp_r):
        ks = pos[:, (r * (nc - 1)) % nc, :].reshape(-1)
        Bx[ks, r] = _signs(rng, ks.shape)
    assert T * amax < 1 << WINDOW_BITS
    c.Bx = Bx[:, :sp_r]
    c.C = exact_product(Ap, Bm, pos, rc, cc)
    c.Cx = Ap @ c.Bx.astype(np.float64)                        # at most T nonzero terms per row, one window: exact in fp64
    return c


def exact_product(Ap, Bm, pos, rc, cc):
    """C = Ap Bm over the census's nonzero positions only (T terms per output), in fp64: exact (the terms are exact, their sums < 2^24 units)."""
    C = np.zeros((Ap.shape[0], Bm.shape[1]))
    for t in range(pos.shape[2]):
        k = pos[rc[:, None], cc[None, :], t]                   # (M, N): the t-th k of output (i, j)
        C += Ap[np.arange(Ap.shape[0])[:, None], k] * Bm[k, np.arange(Bm.shape[1])[None, :]]
    return C


def emulate(a, b, weights=None, acc=np.float32):
    """The split product from pieces: sum over k of the weighted terms a_p[:, k] b_q[k, :], accumulated in `acc` one k and one term at a time.
    a: [3](M, K), b: [3](K, N); weights: {(p, q): w} (default: the six terms, weight 1)."""
    w = dict.fromkeys(TERMS, 1.0) if weights is None else weights
    a, b = [x.astype(acc) for x in a], [x.astype(acc) for x in b]
    C = np.zeros((a[0].shape[0], b[0].shape[1]), acc)
    for k in np.flatnonzero(np.any([x != 0 for x in a], axis=(0, 1)) & np.any([x != 0 for x in b], axis=(0, 2))):
        for (p, q), wt in w.items():
            if wt:
                C += acc(wt) * np.outer(a[p - 1][:, k], b[q - 1][k, :])
    return C

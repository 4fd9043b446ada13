"""fp64 restatement of InteractingLayer (AutoInt's field self-attention), written as the loops of its definition -- per sample, per head, per
query, per key:

    Q = X Wq, K = X Wk, V = X Wv;   s_ij = <Q_i, K_j> over the head's columns (* 1/sqrt(d));   a_ij = exp(s_ij - max_j s_ij) / sum_j ..
    pre_i = sum_j a_ij V_j (+ x_i Wr);   out = relu(pre) or pre

and the backward derived by hand from it (ReLU subgradient 0 at 0):

    dpre = g [pre > 0];   dA_ij = <dpre_i, V_j>;   dV_j += a_ij dpre_i;   dS_ij = a_ij (dA_ij - sum_j' a_ij' dA_ij') (* 1/sqrt(d))
    dQ_i += dS_ij K_j;   dK_j += dS_ij Q_i;   dX = dQ Wq^T + dK Wk^T + dV Wv^T + dpre Wr^T;   dW* = X^T d*

numpy only.  `run` also returns, per sample, the smallest |pre| relative to that sample's largest |pre|; `draw` redraws every sample for which
that ratio is below KINK = 2e-5, twice the tests' output bound, so that a kernel within the bound has every ReLU sign right and no entry has to be
left out of a comparison."""
import numpy as np

KINK = 2e-5


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def run(X, Wq, Wk, Wv, Wr, H, d, scaling=False, relu=True, g=None):
    """X (B, F, D); W* (D, H*d), Wr None without the residual; g (B, F, E) or None.
    Returns dict(out, pre (B, F, E), ratio (B,)) and, with g, dX (B, F, D), dWq, dWk, dWv, dWr (None without Wr)."""
    X, Wq, Wk, Wv, Wr, g = _f64(X), _f64(Wq), _f64(Wk), _f64(Wv), _f64(Wr), _f64(g)
    B, F, D = X.shape
    E = H * d
    scale = 1.0 / np.sqrt(d) if scaling else 1.0
    pre = np.zeros((B, F, E))
    res = dict(dX=np.zeros((B, F, D)), dWq=np.zeros((D, E)), dWk=np.zeros((D, E)), dWv=np.zeros((D, E)),
               dWr=None if Wr is None else np.zeros((D, E))) if g is not None else {}
    if g is not None:
        g = g.reshape(B, F, E)
    for b in range(B):
        x = X[b]
        Q, K, V = x @ Wq, x @ Wk, x @ Wv
        A = np.zeros((H, F, F))
        p = np.zeros((F, E)) if Wr is None else x @ Wr
        for h in range(H):
            hs = slice(h * d, (h + 1) * d)
            for i in range(F):
                s = np.zeros(F)
                for j in range(F):
                    s[j] = np.dot(Q[i, hs], K[j, hs]) * scale
                e = np.exp(s - s.max())
                A[h, i] = e / e.sum()
                for j in range(F):
                    p[i, hs] += A[h, i, j] * V[j, hs]
        pre[b] = p
        if g is None:
            continue
        dp = g[b] * (p > 0) if relu else g[b].copy()
        dQ, dK, dV = np.zeros((F, E)), np.zeros((F, E)), np.zeros((F, E))
        for h in range(H):
            hs = slice(h * d, (h + 1) * d)
            for i in range(F):
                dA = np.zeros(F)
                for j in range(F):
                    dA[j] = np.dot(dp[i, hs], V[j, hs])
                    dV[j, hs] += A[h, i, j] * dp[i, hs]
                rd = np.dot(A[h, i], dA)
                for j in range(F):
                    dS = A[h, i, j] * (dA[j] - rd) * scale
                    dQ[i, hs] += dS * K[j, hs]
                    dK[j, hs] += dS * Q[i, hs]
        res['dX'][b] = dQ @ Wq.T + dK @ Wk.T + dV @ Wv.T + (0.0 if Wr is None else dp @ Wr.T)
        res['dWq'] += x.T @ dQ
        res['dWk'] += x.T @ dK
        res['dWv'] += x.T @ dV
        if Wr is not None:
            res['dWr'] += x.T @ dp
    res['pre'] = pre
    res['out'] = np.maximum(pre, 0.0) if relu else pre
    res['ratio'] = kink_ratio(pre)
    return res


def kink_ratio(pre):
    """Per sample: the smallest |pre| over the largest |pre| (1 for an empty or all-zero sample)."""
    a = np.abs(pre.reshape(len(pre), -1))
    if a.shape[1] == 0:
        return np.ones(len(pre))
    top = a.max(axis=1)
    return np.where(top > 0, a.min(axis=1) / np.where(top > 0, top, 1.0), 1.0)


def pre_einsum(X, Wq, Wk, Wv, Wr, H, d, scaling=False):
    """The same pre by whole-array operations (used by `draw` for the redraw test, and by the CPU tests as a cross-check)."""
    X, Wq, Wk, Wv, Wr = _f64(X), _f64(Wq), _f64(Wk), _f64(Wv), _f64(Wr)
    B, F, _ = X.shape
    Q, K, V = ((X @ W).reshape(B, F, H, d) for W in (Wq, Wk, Wv))
    S = np.einsum('bihc,bjhc->bhij', Q, K) * (1.0 / np.sqrt(d) if scaling else 1.0)
    P = np.exp(S - S.max(-1, keepdims=True))
    A = P / P.sum(-1, keepdims=True)
    O = np.einsum('bhij,bjhc->bihc', A, V).reshape(B, F, H * d)
    return O if Wr is None else O + X @ Wr


def draw(rng, B, F, D, H, d, use_res=True, scaling=False, x_scale=1.0, count=None):
    """The tests' inputs: unit-variance X (times x_scale), weights of std 1/sqrt(D), a unit-variance upstream gradient; float32 arrays.
    Samples whose kink ratio (of the float32 inputs, in fp64) is below KINK are redrawn; `count`, a list, receives (redrawn, drawn)."""
    E = H * d
    Ws = [(rng.standard_normal((D, E)) / np.sqrt(D)).astype(np.float32) for _ in range(4 if use_res else 3)]
    Wr = Ws[3] if use_res else None
    X = (rng.standard_normal((B, F, D)) * x_scale).astype(np.float32)
    redrawn, drawn = 0, B
    for _ in range(200):
        bad = np.nonzero(kink_ratio(pre_einsum(X, Ws[0], Ws[1], Ws[2], Wr, H, d, scaling)) < KINK)[0]
        if len(bad) == 0:
            break
        X[bad] = (rng.standard_normal((len(bad), F, D)) * x_scale).astype(np.float32)
        redrawn += len(bad)
        drawn += len(bad)
    else:
        raise RuntimeError('draw: samples kept landing on the ReLU kink')
    if count is not None:
        count.append((redrawn, drawn))
    g = rng.standard_normal((B, F, E)).astype(np.float32)
    return X, Ws[0], Ws[1], Ws[2], Wr, g


def relrow(got, ref):
    """Worst row of |got - ref| against that row's largest |ref| (rows of zeros: against 1e-30).  NaN anywhere: inf."""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    ref = ref.reshape(len(ref), -1)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    err = np.abs(got - ref).max(axis=1)
    scale = np.maximum(np.abs(ref).max(axis=1), 1e-30)
    worst = (err / scale).max()
    return float(worst) if np.isfinite(worst) else float('inf')


def reltensor(got, ref):
    """|got - ref| against the tensor's largest |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    worst = np.abs(got.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-30)
    return float(worst) if np.isfinite(worst) else float('inf')

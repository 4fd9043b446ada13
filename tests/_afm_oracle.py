"""fp64 restatement of AFMLayer (attentional FM pair pooling), written as the loops of its definition -- per sample, per pair, per hidden unit:

    p_k = x_i * x_j  (pairs k = (i, j), i < j, i-major);   z_k[a] = <W[:, a], p_k> + b[a];   e_k = sum_a relu(z_k[a]) h[a]
    a = exp(e - max e) / sum ..;   v = sum_k a_k p_k;   out = <v, p>  or  v

and the backward derived by hand from it (ReLU subgradient 0 at 0):

    dv = g p (or g);  dp = sum_b g_b v_b;  da_k = <dv, p_k>;  de_k = a_k (da_k - sum_k' a_k' da_k');  dh += de_k relu(z_k)
    dz_k = de_k h [z_k > 0];  db += dz_k;  dW += p_k dz_k^T;  dp_k = a_k dv + W dz_k;  dx_i += dp_k * x_j;  dx_j += dp_k * x_i

numpy only.  `draw` redraws every sample that has a hidden unit with |z| < GATE (sum_c |W_ca p_c| + |b_a|), GATE = 1e-5: an fp32 FMA dot product
of D <= 64 rounded products errs by at most (D + 2) 2^-24 <= 3.9e-6 of that sum, so a kernel has every ReLU gate right and no entry has to be
left out of a comparison."""
import numpy as np

GATE = 1e-5


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def pairs(F):
    return [(i, j) for i in range(F) for j in range(i + 1, F)]


def run(X, W, b, h, p=None, g=None):
    """X (B, F, D); W (D, A); b (A,); h (A,) or (A, 1); p (D,) or (D, 1) or None (no projection); g (B, 1) / (B, D) or None.
    Returns dict(out (B, 1) | (B, D), v (B, D), a (B, P), scale (B,): sum_c |v_c p_c| (the projected output may cancel)) and, with g,
    dX (B, F, D), dW, db, dh (A,), dp (D,) (None without p), db_abs (A,): sum |dz| (db of a unit whose gate is always open is h_a sum_k de_k = 0:
    it cancels exactly)."""
    X, W, b, h, p, g = _f64(X), _f64(W), _f64(b), _f64(h), _f64(p), _f64(g)
    B, F, D = X.shape
    A = W.shape[1]
    h = h.reshape(A)
    p = None if p is None else p.reshape(D)
    pr = pairs(F)
    P = len(pr)
    v = np.zeros((B, D))
    att = np.zeros((B, P))
    res = dict(dX=np.zeros((B, F, D)), dW=np.zeros((D, A)), db=np.zeros(A), db_abs=np.zeros(A), dh=np.zeros(A), dp=None if p is None else np.zeros(D)) if g is not None else {}
    if g is not None:
        g = g.reshape(B, 1 if p is not None else D)
    for s in range(B):
        x = X[s]
        pk = np.zeros((P, D))
        z = np.zeros((P, A))
        e = np.zeros(P)
        for k, (i, j) in enumerate(pr):
            pk[k] = x[i] * x[j]
            for a in range(A):
                z[k, a] = np.dot(W[:, a], pk[k]) + b[a]
                if z[k, a] > 0:
                    e[k] += z[k, a] * h[a]
        if P:
            w = np.exp(e - e.max())
            att[s] = w / w.sum()
        for k in range(P):
            v[s] += att[s, k] * pk[k]
        if g is None or P == 0:
            continue
        dv = g[s, 0] * p if p is not None else g[s].copy()
        if p is not None:
            res['dp'] += g[s, 0] * v[s]
        da = np.array([np.dot(dv, pk[k]) for k in range(P)])
        mean = np.dot(att[s], da)
        for k, (i, j) in enumerate(pr):
            de = att[s, k] * (da[k] - mean)
            dpk = att[s, k] * dv
            for a in range(A):
                if z[k, a] > 0:
                    res['dh'][a] += de * z[k, a]
                    dz = de * h[a]
                    res['db'][a] += dz
                    res['db_abs'][a] += abs(dz)
                    res['dW'][:, a] += pk[k] * dz
                    dpk = dpk + W[:, a] * dz
            res['dX'][s, i] += dpk * x[j]
            res['dX'][s, j] += dpk * x[i]
    res['v'] = v
    res['a'] = att
    res['scale'] = np.abs(v * p).sum(1) if p is not None else np.abs(v).max(1)
    res['out'] = (v @ p).reshape(B, 1) if p is not None else v
    return res


def gate_margin(X, W, b):
    """Per sample: the smallest |z| / (sum_c |W_ca p_c| + |b_a|) over its pairs and hidden units, by whole-array operations (inf without pairs)."""
    X, W, b = _f64(X), _f64(W), _f64(b)
    B, F, _ = X.shape
    if F < 2 or B == 0:
        return np.full(B, np.inf)
    ii, jj = np.triu_indices(F, 1)
    out = np.empty(B)
    step = max(1, (1 << 22) // (len(ii) * X.shape[2]))
    for s in range(0, B, step):
        pk = X[s:s + step, ii] * X[s:s + step, jj]
        z = pk @ W + b
        mag = np.abs(pk) @ np.abs(W) + np.abs(b)
        out[s:s + step] = np.where(mag > 0, np.abs(z) / np.where(mag > 0, mag, 1.0), np.inf).reshape(len(pk), -1).min(1)
    return out


def draw(rng, B, F, D, A, projection=True, h_scale=1.0, count=None):
    """The tests' inputs: unit-variance X, W of std 1/sqrt(D), b of std 0.1, h (A,) and p (D,) of std 1/sqrt(A) and 1/sqrt(D), a unit-variance
    upstream gradient; float32 arrays.  Samples whose gate margin (of the float32 inputs, in fp64) is below GATE are redrawn; `count`, a list,
    receives (redrawn, drawn).  Returns X, W, b, h, p (None without the projection), g."""
    W = (rng.standard_normal((D, A)) / np.sqrt(D)).astype(np.float32)
    b = (rng.standard_normal(A) * 0.1).astype(np.float32)
    h = (rng.standard_normal(A) / np.sqrt(A) * h_scale).astype(np.float32)
    p = (rng.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    X = rng.standard_normal((B, F, D)).astype(np.float32)
    redrawn, drawn = 0, B
    for _ in range(400):
        bad = np.nonzero(gate_margin(X, W, b) < GATE)[0]
        if len(bad) == 0:
            break
        X[bad] = rng.standard_normal((len(bad), F, D)).astype(np.float32)
        redrawn += len(bad)
        drawn += len(bad)
    else:
        raise RuntimeError('draw: samples kept landing on a ReLU gate')
    if count is not None:
        count.append((redrawn, drawn))
    g = rng.standard_normal((B, 1 if projection else D)).astype(np.float32)
    return X, W, b, h, (p if projection else None), g


def relrow(got, ref):
    """Worst row of |got - ref| against that row's largest |ref| (rows of zeros: against 1e-30).  NaN anywhere: inf."""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    ref = ref.reshape(len(ref), -1)
    return relscale(got, ref, np.abs(ref).max(axis=1))


def relscale(got, ref, scale):
    """Worst row of |got - ref| against that row's `scale` (a zero scale: against 1e-30).  NaN anywhere: inf."""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    ref = ref.reshape(len(ref), -1)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    worst = (np.abs(got - ref).max(axis=1) / np.maximum(np.asarray(scale, dtype=np.float64), 1e-30)).max()
    return float(worst) if np.isfinite(worst) else float('inf')


def reltensor(got, ref):
    """|got - ref| against the tensor's largest |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    worst = np.abs(got.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-30)
    return float(worst) if np.isfinite(worst) else float('inf')

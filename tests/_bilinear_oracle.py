"""fp64 restatement of BilinearInteractionLayer (FiBiNET's bilinear cross), written as the three loops of its definition:

    out[b, p*D:(p+1)*D] = (x_i[b] @ W[w(p)]) * x_j[b]      pairs p = (i, j), i < j, i-major;  w(p) = 0 / i / p

    dX_j += g_ij * U_i,   dU_i = g_ij * x_j,   dX_i += dU_i @ W[w]^T,   dW[w] += x_i^T dU_i

numpy only; the tests' reference for out, dX per field and dW, and the row-wise error measure `relrow`."""
import numpy as np

TYPES = ('all', 'each', 'interaction')


def pairs(F):
    return [(i, j) for i in range(F) for j in range(i + 1, F)]


def n_weights(kind, F):
    return {'all': 1, 'each': max(F - 1, 1), 'interaction': max(F * (F - 1) // 2, 1)}[kind]


def w_index(kind, p, i):
    return {'all': 0, 'each': i, 'interaction': p}[kind]


def forward(xs, W, kind):
    """xs: list of F (B, D) arrays, W (nW, D, D).  Returns (B, P*D) float64."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    W = np.asarray(W, dtype=np.float64)
    B, D = xs[0].shape
    prs = pairs(len(xs))
    out = np.zeros((B, len(prs) * D))
    for p, (i, j) in enumerate(prs):
        out[:, p * D:(p + 1) * D] = (xs[i] @ W[w_index(kind, p, i)]) * xs[j]
    return out


def backward(xs, W, kind, g):
    """g (B, P*D): the gradient of the output.  Returns ([dX_f (B, D)], dW (nW, D, D)) in float64."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    W = np.asarray(W, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    B, D = xs[0].shape
    dxs = [np.zeros((B, D)) for _ in xs]
    dW = np.zeros_like(W)
    for p, (i, j) in enumerate(pairs(len(xs))):
        w = w_index(kind, p, i)
        gp = g[:, p * D:(p + 1) * D]
        dxs[j] += gp * (xs[i] @ W[w])
        du = gp * xs[j]
        dxs[i] += du @ W[w].T
        dW[w] += xs[i].T @ du
    return dxs, dW


def relrow(got, ref):
    """Worst row of |got - ref| against that row's largest |ref| (rows of zeros: against 1e-30).  NaN anywhere: inf."""
    got = np.asarray(got, dtype=np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref).max(axis=1)
    scale = np.maximum(np.abs(ref).max(axis=1), 1e-30)
    worst = (err / scale).max()
    return float(worst) if np.isfinite(worst) else float('inf')


def reltensor(got, ref):
    """|got - ref| against the tensor's largest |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    return float(worst) if np.isfinite(worst) else float('inf')


def draw(rng, B, F, D, kind):
    """The tests' inputs: unit-variance rows, W of std 1/sqrt(D), a unit-variance upstream gradient.  float32 arrays."""
    xs = [rng.standard_normal((B, D)).astype(np.float32) for _ in range(F)]
    W = (rng.standard_normal((n_weights(kind, F), D, D)) / np.sqrt(D)).astype(np.float32)
    g = rng.standard_normal((B, F * (F - 1) // 2 * D)).astype(np.float32)
    return xs, W, g

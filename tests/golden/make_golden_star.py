"""Regenerates tests/golden/{star_dense,parasitic_star,stacked_dense,parasitic_stacked}.npz.  Run from the repo root:
python tests/golden/make_golden_star.py

As tests/golden/make_golden.py: the inputs and weights of the reference's own StarDense / StackedDense unit tests, regenerated with
oracle/tf_seeded_rng.py, plus the literal goldens those tests assert (transcribed DATA, cited by file:line below).  The parameter
tables are ones / zeros, so the scene draw does not matter, and ops with explicit seeds take no op seed from the global stream.  A
fixture is written only when the fp64 oracle (tests/_star_oracle.py) reproduces its golden within sum|diff| < 1e-5.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import dense_ref as R                      # noqa: E402
import _star_oracle as S                   # noqa: E402
from tf_seeded_rng import TFSeededRNG      # noqa: E402

T = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
TOL = 1e-5
ADAM = dict(lr=0.005, beta1=0.9, beta2=0.999, eps=1e-7)     # tf.keras.optimizers.Adam(0.005) defaults


def _check(name, golden, got):
    diff = R.calc_sum_of_abs_diff(got, golden)
    assert diff < TOL, '%s: oracle does not reproduce the reference golden (sum|diff| = %g)' % (name, diff)
    print('%-18s sum|oracle-golden| = %.3g' % (name, diff))


def star_dense():
    # tests/layers/test_star_dense_layer.py:21-47 (ones table: every parameter row is ones)
    r = TFSeededRNG(1)
    x = r.uniform([2, 3], 0.0, 1.0, seed=1)
    kernel = r.glorot_uniform([3, 5])
    bias = np.zeros(5, np.float32)
    params = np.ones((2, 3 * 5 + 5), np.float32)
    golden = [[-0.0108437, 0.06807042, 0.05824887, 0.01455763, -0.01269773],
              [0.14119211, 0.8420988, 0.3796606, 0.27883598, 0.05301704]]
    _check('star_dense', golden, S.star_dense(T(x), T(kernel), T(bias), [T(params)]).numpy())
    np.savez(os.path.join(HERE, 'star_dense.npz'), golden=np.float32(golden), inputs=x, kernel=kernel, bias=bias, params=params)


def adam_steps(x, kernel, bias, group_idx, steps, lr, beta1, beta2, eps):
    """Keras Adam on the parasitic kernel / bias of a ParasiticStarDenseLayer with a frozen trunk (ones / zeros initialised):
    m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, var -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps).  Returns
    (parasitic kernel, parasitic bias, the loss of the last step)."""
    pk = torch.ones((2,) + tuple(kernel.shape), dtype=torch.float64, requires_grad=True)
    pb = torch.zeros((2,) + tuple(bias.shape), dtype=torch.float64, requires_grad=True)
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in (pk, pb)]
    for t in range(1, steps + 1):
        y = S.parasitic_dense(x, kernel, bias, pk, pb, group_idx, 'star')
        loss = ((y - 1.0) ** 2).sum(1).mean()
        gk, gb = torch.autograd.grad(loss, (pk, pb))
        with torch.no_grad():
            step = lr * (1 - beta2 ** t) ** 0.5 / (1 - beta1 ** t)
            for p, g, (m, v) in zip((pk, pb), (gk, gb), state):
                m.mul_(beta1).add_((1 - beta1) * g)
                v.mul_(beta2).add_((1 - beta2) * g * g)
                p.sub_(step * m / (v.sqrt() + eps))
    return pk.detach(), pb.detach(), loss.detach()


def parasitic_star():
    # tests/layers/test_star_dense_layer.py:52-76 (groups 0 and 1 of a ones-initialised parasitic kernel)
    r = TFSeededRNG(1)
    x = r.uniform([2, 3], 0.0, 1.0, seed=1)
    kernel = r.glorot_uniform([3, 4])
    bias = np.zeros(4, np.float32)
    golden = [[-0.02065258, 0.0599786, 0.04785775, 0.00602703],
              [-0.24781615, 0.4868825, 0.78814316, 0.0116475]]
    pk, pb = torch.ones(5, 3, 4, dtype=torch.float64), torch.zeros(5, 4, dtype=torch.float64)
    for g in (0, 1):
        _check('parasitic_star/%d' % g, golden, S.parasitic_dense(T(x), T(kernel), T(bias), pk, pb, g, 'star').numpy())
    # tests/layers/test_star_dense_layer.py:78-107 (3 Adam steps on group 1, trunk frozen, U = 1)
    r = TFSeededRNG(1)
    xg = r.uniform([2, 3], 0.0, 1.0, seed=1)
    kg = r.glorot_uniform([3, 1])
    bg = np.zeros(1, np.float32)
    golden_kernel = [[[1.], [1.], [1.]], [[0.9850103], [1.0149864], [1.0149883]]]
    golden_bias = [[0.], [0.01499427]]
    golden_loss = 0.56336486
    gk, gb, loss = adam_steps(T(xg), T(kg), T(bg), 1, 3, **ADAM)
    _check('parasitic_star/k', golden_kernel, gk.numpy())
    _check('parasitic_star/b', golden_bias, gb.numpy())
    _check('parasitic_star/l', golden_loss, loss.numpy())
    np.savez(os.path.join(HERE, 'parasitic_star.npz'), golden=np.float32(golden), inputs=x, kernel=kernel, bias=bias,
             grad_inputs=xg, grad_kernel=kg, grad_bias=bg, golden_parasitic_kernel=np.float32(golden_kernel),
             golden_parasitic_bias=np.float32(golden_bias), golden_loss=np.float32(golden_loss))


def stacked_dense():
    # tests/layers/test_stacked_dense_layer.py:21-47 (zeros table)
    r = TFSeededRNG(1)
    x = r.uniform([2, 3], 0.0, 1.0, seed=1)
    kernel = r.glorot_uniform([3, 5])
    bias = np.zeros(5, np.float32)
    params = np.zeros((2, 3 * 5 + 5), np.float32)
    golden = [[-0.0108437, 0.06807042, 0.05824887, 0.01455763, -0.01269773],
              [0.14119211, 0.8420988, 0.3796606, 0.27883598, 0.05301704]]
    _check('stacked_dense', golden, S.stacked_dense(T(x), T(kernel), T(bias), [T(params)]).numpy())
    np.savez(os.path.join(HERE, 'stacked_dense.npz'), golden=np.float32(golden), inputs=x, kernel=kernel, bias=bias, params=params)


def parasitic_stacked():
    # tests/layers/test_stacked_dense_layer.py:52-66 (parasitic kernel initialised to ones, group 0)
    r = TFSeededRNG(0)
    x = r.uniform([2, 2], 0.0, 1.0, seed=1)
    kernel = r.glorot_uniform([2, 3])
    bias = np.zeros(3, np.float32)
    golden = [[0.41276646, 0.2785303, 0.75729215],
              [1.1768938, 0.84114075, 1.7925735]]
    pk, pb = torch.ones(1, 2, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64)
    _check('parasitic_stacked', golden, S.parasitic_dense(T(x), T(kernel), T(bias), pk, pb, 0, 'stacked').numpy())
    np.savez(os.path.join(HERE, 'parasitic_stacked.npz'), golden=np.float32(golden), inputs=x, kernel=kernel, bias=bias)


if __name__ == '__main__':
    star_dense()
    parasitic_star()
    stacked_dense()
    parasitic_stacked()

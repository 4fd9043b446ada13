"""Regenerates tests/golden/attention_dnn.npz.  Run from the repo root:  python tests/golden/make_golden_din.py

The inputs of the reference's own unit test (tests/rec_block/test_attention.py:57-67: literal user / doc embeddings,
tf.random.set_seed(0), dnn_dims [32, 24, 1]), its three Dense kernels regenerated with oracle/tf_seeded_rng.py (glorot_uniform of
[4, 32], [32, 24], [24, 1] in layer order, zero biases: keras.layers.Dense defaults), and the literal goldens that test asserts
(:69-70, transcribed DATA).  The fixture is written only when the fp64 oracle (tests/_din_oracle.py) reproduces both goldens within
sum|diff| < 1e-5, the reference test's own tolerance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import dense_ref as R                      # noqa: E402
import _din_oracle as O                    # noqa: E402
from tf_seeded_rng import TFSeededRNG      # noqa: E402

T = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
TOL = 1e-5


def main():
    # tests/rec_block/test_attention.py:59-64
    user = np.array([[[0.1, 0.2], [-0.1, -0.2]], [[0.3, 0.4], [-0.3, -0.4]]], np.float32)
    doc = np.array([[0.1, 0.2], [0.3, 0.4]], np.float32)
    dims = [32, 24, 1]
    r = TFSeededRNG(0)
    kernels, width = [], 2 * user.shape[2]
    for d in dims:
        kernels.append(r.glorot_uniform([width, d]))
        width = d
    biases = [np.zeros(d, np.float32) for d in dims]
    # :69-70
    golden_mat = [[0.00044473, 0.00088945], [0.00321232, 0.0042831]]
    golden_sum = [[0.9462962], [0.8750266]]
    mat, ssum = O.attention_by_dnn(T(user), T(doc), [T(k) for k in kernels], [T(b) for b in biases])
    for name, g, got in (('attn_mat', golden_mat, mat), ('attn_score_sum', golden_sum, ssum)):
        diff = R.calc_sum_of_abs_diff(got.numpy(), g)
        assert diff < TOL, '%s: oracle does not reproduce the reference golden (sum|diff| = %g)' % (name, diff)
        print('%-15s sum|oracle-golden| = %.3g' % (name, diff))
    out = dict(user=user, doc=doc, dims=np.int32(dims), golden_mat=np.float32(golden_mat), golden_sum=np.float32(golden_sum))
    for i, (k, b) in enumerate(zip(kernels, biases)):
        out['kernel%d' % i], out['bias%d' % i] = np.float32(k), b
    np.savez(os.path.join(HERE, 'attention_dnn.npz'), **out)


if __name__ == '__main__':
    main()

"""Regenerates tests/golden/sparse_gnn.npz.  Run from the repo root:  python tests/golden/make_golden_gnn.py

The input of the reference's own SparseGNNLayer unit test (tests/layers/test_sparse_gnn_layer.py:19-26: tf.random.set_seed(1), then
random_normal_initializer()([2, 3, 4])), regenerated with oracle/tf_seeded_rng.py, and the literal golden that test asserts (:35-43,
transcribed DATA).  The fixture is written only when the fp64 oracle (tests/_gnn_oracle.py) reproduces the golden within
sum|diff| < 1e-5, the reference test's own bound.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import _gnn_oracle as G                    # noqa: E402
from tf_seeded_rng import TFSeededRNG      # noqa: E402

TOL = 1e-5


def main():
    x = TFSeededRNG(1).random_normal_initializer([2, 3, 4]).astype(np.float32)      # (B, F, D)
    fields = [0, 1, 2]
    field2neighbors = {0: [2], 1: [2, 0]}
    golden = np.array([[[-0.06320834, -0.08645303, -0.02788609],
                        [0.06614043, -0.03772061, -0.03598052],
                        [0.00979297, -0.00018102, -0.031269],
                        [-0.0545692, -0.03511687, -0.03570567]],
                       [[-0.01362271, 0.06267785, 0.01263753],
                        [-0.00716899, 0.00449803, 0.03215501],
                        [0.04116546, 0.02203641, 0.10609905],
                        [0.04295323, 0.02166578, -0.04118742]]], np.float32)           # (B, D, F)
    indices = G.sorted_indices(fields, field2neighbors)
    assert indices == [[0, 1], [2, 0], [2, 1]], indices
    weights = [torch.full((len(indices),), 0.1, dtype=torch.float64) for _ in range(3)]
    got = G.sparse_gnn_bfd(torch.from_numpy(x).double(), indices, weights, 3, 'tanh')[-1].numpy()
    diff = float(np.abs(got - golden).sum())
    assert diff < TOL, 'oracle does not reproduce the reference golden (sum|diff| = %g)' % diff
    print('sparse_gnn         sum|oracle-golden| = %.3g' % diff)
    np.savez(os.path.join(HERE, 'sparse_gnn.npz'), inputs=x, golden=golden, indices=np.array(indices, np.int64),
             num_layers=np.int64(3), weight=np.float32(0.1))


if __name__ == '__main__':
    main()

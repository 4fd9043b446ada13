"""Regenerates tests/golden/can.npz.  Run from the repo root:  python tests/golden/make_golden_can.py

As tests/golden/make_golden_star.py: the inputs of the reference's own CANLayer unit test, regenerated with oracle/tf_seeded_rng.py, plus
the literal values that test asserts (transcribed DATA, cited by file:line below).  The fixture is written only when the fp64 oracle
(tests/_can_oracle.py) reproduces the golden within sum|diff| < 1e-5.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import dense_ref as R                      # noqa: E402
import _can_oracle as C                    # noqa: E402
from tf_seeded_rng import TFSeededRNG      # noqa: E402

T = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
TOL = 1e-5


def can():
    # tests/layers/test_can_layer.py:27-51: tf.random.set_seed(1); two unseeded random_normal_initializer() draws in program order
    dims = [4, 3, 2]
    r = TFSeededRNG(1)
    inputs = r.random_normal_initializer([2, 3, 4])
    params = r.random_normal_initializer([2, C.param_size(4, dims)])
    golden = [[0.06818546, 0.12346052],
              [0.11372094, 0.23575373]]
    got = C.can_layer(T(inputs), T(params), dims).numpy()
    diff = R.calc_sum_of_abs_diff(got, golden)
    assert diff < TOL, 'can: oracle does not reproduce the reference golden (sum|diff| = %g)' % diff
    print('can                sum|oracle-golden| = %.3g' % diff)
    # tests/layers/test_can_layer.py:18-25
    nz_inputs = np.float32([[[1, 2, 0], [0, 0, 0]], [[1, 0, 0], [0, 0, 0.1]]])
    nz_golden = np.array([[[True], [False]], [[True], [True]]])
    np.savez(os.path.join(HERE, 'can.npz'), golden=np.float32(golden), inputs=inputs, params=params, dims=np.int32(dims),
             nz_inputs=nz_inputs, nz_golden=nz_golden)


if __name__ == '__main__':
    can()

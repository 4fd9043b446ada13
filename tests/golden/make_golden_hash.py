"""Writes tests/golden/multi_hash.npz: inputs, embedding tables and expected outputs of the eight unit tests of the reference's MultiHashLayer and
FastMultiHashLayer (tests/layers/test_multi_hash_layer.py, test_fast_multi_hash_layer.py).  Data only.

The expected outputs are the literals of those tests.  The tables are what `tf.random.set_seed(1)` + `random_normal_initializer()` give the
layers, regenerated without TensorFlow by oracle/tf_seeded_rng.py: MultiHashLayer builds three (10, 2) tables in turn (three successive draws),
FastMultiHashLayer one (30, 2) table.

    python tests/golden/make_golden_hash.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
from tf_seeded_rng import TFSeededRNG  # noqa: E402

STR_INPUTS = [['Aa', 'Bb'], ['Cc', 'Dd'], ['Ee', 'Ff']]
INT_INPUTS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14]]

MULTI_CONCAT = [[[-0.05506101, 0.07728758, -0.01676805, -0.05213338, 0.03821649, -0.04180959],
                 [-0.01598444, 0.01866628, -0.03418445, 0.03368045, -0.08921313, -0.02610026]],
                [[0.0191822, -0.04398289, -0.03821107, -0.05186243, 0.05728074, 0.01030363],
                 [-0.01741772, -0.01682349, 0.05045691, 0.0618127, 0.01563057, 0.04971462]],
                [[-0.01598444, 0.01866628, -0.01676805, -0.05213338, 0.03821649, -0.04180959],
                 [-0.05506101, 0.07728758, 0.05045691, 0.0618127, -0.00986082, 0.02690467]]]
MULTI_SUM = [[[-0.03361257, -0.01665538], [-0.13938202, 0.02624647]],
             [[0.03825187, -0.0855417], [0.04866976, 0.09470383]],
             [[0.005464, -0.07527669], [-0.01446492, 0.16600496]]]
MULTI_POOLING = [[-0.08649729, 0.00479554], [0.04346082, 0.00458107], [-0.00450046, 0.04536413]]
MULTI_NO_EMB = [[809, 954, 690, 178, 168, 578], [859, 941, 233, 230, 311, 20], [9, 228, 330, 245, 394, 369], [374, 713, 248, 70, 185, 525],
                [472, 521, 568, 664, 41, 462], [621, 123, 902, 156, 860, 822], [621, 63, 659, 926, 792, 165]]

FAST_CONCAT = [[-0.03129962, -0.0357513, -0.03292613, -0.04916694, 0.00508573, -0.05960856, -0.05506101, 0.07728758, -0.07800285, -0.00789563,
                -0.00520009, -0.03755732],
               [0.06398293, -0.00107379, 0.06124375, 0.00293248, 0.00845301, 0.05227221, 0.00439039, -0.01016302, 0.01944189, -0.05186224,
                0.05924026, -0.01769078],
               [0.00439039, -0.01016302, -0.03292613, -0.04916694, 0.00508573, -0.05960856, -0.06123361, -0.04905606, 0.01944189, -0.05186224,
                0.04603096, -0.01844464]]
FAST_SUM = [[[-0.05914002, -0.1445268], [-0.13826394, 0.03183464]],
            [[0.1336797, 0.0541309], [0.08307254, -0.07971604]],
            [[-0.02345001, -0.11893852], [0.00423924, -0.11936294]]]
FAST_POOLING = [[-0.09870198, -0.05634608], [0.10837612, -0.01279257], [-0.00960538, -0.11915073]]
FAST_NO_EMB = [[849, 759, 690, 178, 168, 578], [921, 543, 233, 230, 311, 20], [971, 487, 330, 245, 394, 369], [88, 627, 248, 70, 185, 525],
               [85, 862, 568, 664, 41, 462], [439, 888, 902, 156, 860, 822], [843, 665, 659, 926, 792, 165]]


def main():
    rng = TFSeededRNG(1)
    multi_tables = np.stack([np.asarray(rng.random_normal_initializer((10, 2)), dtype=np.float32) for _ in range(3)])
    fast_table = np.asarray(TFSeededRNG(1).random_normal_initializer((30, 2)), dtype=np.float32)
    np.savez(os.path.join(HERE, 'multi_hash.npz'),
             str_inputs=np.array(STR_INPUTS, dtype='S2'), int_inputs=np.array(INT_INPUTS, dtype=np.int64),
             num_bins_emb=np.int64(10), num_bins_no_emb=np.int64(1000), num_hash=np.int64(3), salts=np.int64(1), pooling_weight=np.float32(0.5),
             multi_tables=multi_tables, fast_table=fast_table,
             multi_concat=np.array(MULTI_CONCAT, dtype=np.float32), multi_sum=np.array(MULTI_SUM, dtype=np.float32),
             multi_pooling=np.array(MULTI_POOLING, dtype=np.float32), multi_no_emb=np.array(MULTI_NO_EMB, dtype=np.int64),
             fast_concat=np.array(FAST_CONCAT, dtype=np.float32), fast_sum=np.array(FAST_SUM, dtype=np.float32),
             fast_pooling=np.array(FAST_POOLING, dtype=np.float32), fast_no_emb=np.array(FAST_NO_EMB, dtype=np.int64))


if __name__ == '__main__':
    main()

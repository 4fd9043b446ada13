"""Writes tests/golden/tensor_util.npz: the literal inputs and expected outputs of the reference's unit tests of PoolingLayer
(tests/layers/test_pooling_layer.py, 2 cases), FixLengthLayer (tests/layers/test_fix_length_layer.py, 3 cases; length 2, axis -1) and
gather_embedding_element_wise_weight (tests/rec_block/test_embedding_wise_weight.py, 1 case).  Data only; the weights the reference's test
derives (range(num_embedding * batch_size) + 10, reshaped) are stored already derived.

    python tests/golden/make_golden_tensor_util.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

POOL_IN = [[1, 2, 3], [10, 11, 12]]
POOL_AXIS0_KEEPDIMS_SUM = [[11, 13, 15]]
POOL_AXIS1_SUM = [6, 33]

FIX_TRUNCATE_IN = [[1, 2, 3], [4, 5, 6]]
FIX_TRUNCATE_OUT = [[1, 2], [4, 5]]
FIX_PAD_IN = [[1], [2]]
FIX_PAD_OUT = [[1, 0], [2, 0]]
FIX_SAME_IN = [[1, 2], [3, 4]]
FIX_SAME_OUT = [[1, 2], [3, 4]]

ELW_POS_IDX = [0, 1, 1, 2, 2, 2]
ELW_BATCH = 4
ELW_OUT = [[10, 11, 11, 12, 12, 12],
           [13, 14, 14, 15, 15, 15],
           [16, 17, 17, 18, 18, 18],
           [19, 20, 20, 21, 21, 21]]


def main():
    f32 = np.float32
    num_embedding = max(ELW_POS_IDX) + 1
    np.savez(os.path.join(HERE, 'tensor_util.npz'),
             pool_in=np.array(POOL_IN, dtype=f32), pool_axis0_keepdims_sum=np.array(POOL_AXIS0_KEEPDIMS_SUM, dtype=f32),
             pool_axis1_sum=np.array(POOL_AXIS1_SUM, dtype=f32),
             fix_length=np.int64(2), fix_axis=np.int64(-1),
             fix_truncate_in=np.array(FIX_TRUNCATE_IN, dtype=f32), fix_truncate_out=np.array(FIX_TRUNCATE_OUT, dtype=f32),
             fix_pad_in=np.array(FIX_PAD_IN, dtype=f32), fix_pad_out=np.array(FIX_PAD_OUT, dtype=f32),
             fix_same_in=np.array(FIX_SAME_IN, dtype=f32), fix_same_out=np.array(FIX_SAME_OUT, dtype=f32),
             elw_pos_idx=np.array(ELW_POS_IDX, dtype=np.int32),
             elw_weights=(np.arange(num_embedding * ELW_BATCH) + 10).reshape(ELW_BATCH, num_embedding).astype(f32),
             elw_out=np.array(ELW_OUT, dtype=f32))


if __name__ == '__main__':
    main()

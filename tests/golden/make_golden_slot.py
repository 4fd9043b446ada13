"""Writes tests/golden/slot_util.npz: the literal inputs and expected outputs of the unit tests of the reference's rec_block/embedding_util.py
(tests/rec_block/test_embedding_util.py) for isin, mask_values, first_occurance_in_row, batch_segment_ids_of_targets, embedding_single_slot,
pool_slots (both cases), pool_single_slot and fetch_single_slot (both cases).  Data only: inputs that the reference's tests derive from others
(slots = int((ids + 0.5) / 10), weights = ids * 10, ids = slots * 10 + offsets, weights = slots * 0.1) are stored already derived.

    python tests/golden/make_golden_slot.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MAT = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]
TARGET_VALUES = [1, 3, 5, 7, 9]
ISIN = [[False, True, False, True, False], [True, False, True, False, True]]
MASK_VALUES = [[-1, 1, -1, 3, -1], [5, -1, 7, -1, 9]]

SEG_SLOTS = [[0, 1, 1, 2, 3, 3], [1, 3, 3, 2, 5, 5]]
FIRST_OCCURANCE = [[0, 1, -1, 2, 3, -1], [1, 3, -1, 2, 5, -1]]
SEG_TARGETS = [1, 3, 5]
BATCH_SEGMENT_IDS = [[-1, 0, 0, -1, 1, 1], [3, 4, 4, -1, 5, 5]]

EMB_IDS = [[0, 10, 10, 30], [21, 22, 31, 1]]
EMB_OUT = [[[0., 0.], [0., 0.]], [[21., -21.], [22., -22.]]]
EMB_WEIGHTS = [[[0.], [0.]], [[210.], [220.]]]
EMB_MASK = [[[False], [False]], [[True], [True]]]

POOL_SLOTS = [[1, 2, 3, 0, 0], [2, 2, 4, 5, 0]]
POOL_ID_OFFSETS = [[0, 0, 0, 0, 0], [8, 0, 0, 0, 0]]
POOL_IDS_KEEP = [[20, 30], [20, 0]]
POOL_WEIGHTS_KEEP = [[0.2, 0.3], [0.4, 0.]]
POOL_IDS_DROP = [[20, 30], [28, 0]]
POOL_WEIGHTS_DROP = [[0.2, 0.3], [0.2, 0.]]

SINGLE_SLOTS = [[1, 2, 3], [2, 3, 4]]
SINGLE_IDS = [[20], [20]]
SINGLE_WEIGHTS = [[0.2], [0.2]]

FETCH_IDS = [[0, 10, 11, 30], [21, 22, 31, 1]]
FETCH_OUT_IDS_0 = [[10, 11], [0, 0]]
FETCH_OUT_WEIGHTS_0 = [[100., 110.], [0., 0.]]
FETCH_OUT_IDS_1 = [[10, 11], [10, 10]]
FETCH_OUT_WEIGHTS_1 = [[100., 110.], [1., 1.]]


def slots_of(ids):
    return ((np.asarray(ids, dtype=np.float64) + 0.5) / 10.0).astype(np.int32)


def main():
    i64, i32, f32 = np.int64, np.int32, np.float32
    emb_ids, fetch_ids = np.array(EMB_IDS, dtype=i64), np.array(FETCH_IDS, dtype=i64)
    pool_slots = np.array(POOL_SLOTS, dtype=i32)
    single_slots = np.array(SINGLE_SLOTS, dtype=i32)
    np.savez(os.path.join(HERE, 'slot_util.npz'),
             mat=np.array(MAT, dtype=i32), target_values=np.array(TARGET_VALUES, dtype=i64), isin=np.array(ISIN), mask_padding=i64(-1),
             mask_values=np.array(MASK_VALUES, dtype=i32),
             seg_slots=np.array(SEG_SLOTS, dtype=i32), first_padding=i64(-1), first_occurance=np.array(FIRST_OCCURANCE, dtype=i32),
             seg_targets=np.array(SEG_TARGETS, dtype=i64), batch_segment_ids=np.array(BATCH_SEGMENT_IDS, dtype=i32),
             seg_num_rows=i64(2), seg_num_ids=i64(3), seg_num_segments=i64(6),
             emb_table=np.array([[i, -i] for i in range(40)], dtype=f32), emb_ids=emb_ids, emb_slots=slots_of(emb_ids), emb_target=i64(2),
             emb_weights=emb_ids.astype(f32) * f32(10.0), emb_out=np.array(EMB_OUT, dtype=f32), emb_out_weights=np.array(EMB_WEIGHTS, dtype=f32),
             emb_out_mask=np.array(EMB_MASK),
             pool_slots=pool_slots, pool_ids=pool_slots * 10 + np.array(POOL_ID_OFFSETS, dtype=i32), pool_weights=pool_slots.astype(f32) * f32(0.1),
             pool_targets=np.array([2, 3], dtype=i64), pool_ids_keep=np.array(POOL_IDS_KEEP, dtype=i32),
             pool_weights_keep=np.array(POOL_WEIGHTS_KEEP, dtype=f32), pool_ids_drop=np.array(POOL_IDS_DROP, dtype=i32),
             pool_weights_drop=np.array(POOL_WEIGHTS_DROP, dtype=f32),
             single_slots=single_slots, single_ids_in=single_slots * 10, single_weights_in=single_slots.astype(f32) * f32(0.1), single_target=i64(2),
             single_ids=np.array(SINGLE_IDS, dtype=i32), single_weights=np.array(SINGLE_WEIGHTS, dtype=f32),
             fetch_ids=fetch_ids, fetch_slots=slots_of(fetch_ids), fetch_target=i64(1), fetch_weights=fetch_ids.astype(f32) * f32(10.0),
             fetch_default_id_1=i64(10), fetch_default_weight_1=f32(1.0),
             fetch_out_ids_0=np.array(FETCH_OUT_IDS_0, dtype=i64), fetch_out_weights_0=np.array(FETCH_OUT_WEIGHTS_0, dtype=f32),
             fetch_out_ids_1=np.array(FETCH_OUT_IDS_1, dtype=i64), fetch_out_weights_1=np.array(FETCH_OUT_WEIGHTS_1, dtype=f32))


if __name__ == '__main__':
    main()

"""The fixture cases of tests/golden/slot_util.npz (the reference's own unit tests of rec_block/embedding_util.py), written once and run against
two implementations: the numpy oracle (tests/test_slot_util_cpu.py) and the public GPU functions (tests/test_slot_util_gpu.py).

`api` is a namespace with the reference's function names; `put` moves a numpy input to where the implementation wants it; `get` brings an output
back as numpy; `embedding_func(table)` builds the lookup handed to embedding_single_slot.  Integer and bool outputs must be equal, float outputs
within the reference tests' own criterion: sum of absolute differences < 1e-5."""
import warnings

import numpy as np

SUM_ABS_BOUND = 1e-5


def _equal(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    assert np.array_equal(got, want), '%s: %s, expected %s' % (what, got.tolist(), want.tolist())


def _close(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).sum())
    print('%s: sum of absolute differences %.3g' % (what, d))
    assert d < SUM_ABS_BOUND, '%s: sum of absolute differences %.3g' % (what, d)


def run_fixture_cases(g, api, put, get, embedding_func):
    tl = lambda a: [int(v) for v in a]      # noqa: E731
    # isin, mask_values
    _equal(get(api.isin(put(g['mat']), tl(g['target_values']))), g['isin'], 'isin')
    _equal(get(api.mask_values(put(g['mat']), tl(g['target_values']), padding_value=int(g['mask_padding']))), g['mask_values'], 'mask_values')
    # first_occurance_in_row
    _equal(get(api.first_occurance_in_row(put(g['seg_slots']), padding_value=int(g['first_padding']))), g['first_occurance'], 'first_occurance_in_row')
    # batch_segment_ids_of_targets
    seg, nrows, nids, nseg = api.batch_segment_ids_of_targets(put(g['seg_slots']), tl(g['seg_targets']))
    _equal(get(seg), g['batch_segment_ids'], 'batch_segment_ids')
    assert (int(nrows), int(nids), int(nseg)) == (int(g['seg_num_rows']), int(g['seg_num_ids']), int(g['seg_num_segments']))
    # embedding_single_slot
    emb, w, m = api.embedding_single_slot(embedding_func(g['emb_table']), put(g['emb_slots']), int(g['emb_target']), put(g['emb_ids']),
                                          put(g['emb_weights']))
    _close(get(emb), g['emb_out'], 'embedding_single_slot embedding_tensor')
    _close(get(w), g['emb_out_weights'], 'embedding_single_slot weights_tensor')
    _equal(get(m), g['emb_out_mask'], 'embedding_single_slot mask_tensor')
    # pool_slots, both cases
    for drop, tag in ((False, 'keep'), (True, 'drop')):
        pi, pw = api.pool_slots(put(g['pool_slots']), tl(g['pool_targets']), put(g['pool_ids']), put(g['pool_weights']), drop_duplicate_slot=drop)
        _equal(get(pi), g['pool_ids_' + tag], 'pool_slots pooled_ids (drop_duplicate_slot=%s)' % drop)
        _close(get(pw), g['pool_weights_' + tag], 'pool_slots pooled_weights (drop_duplicate_slot=%s)' % drop)
    # pool_single_slot
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        si, sw = api.pool_single_slot(put(g['single_slots']), int(g['single_target']), put(g['single_ids_in']), put(g['single_weights_in']))
    _equal(get(si), g['single_ids'], 'pool_single_slot ids')
    _close(get(sw), g['single_weights'], 'pool_single_slot weights')
    # fetch_single_slot, both cases
    fi, fw = api.fetch_single_slot(put(g['fetch_slots']), int(g['fetch_target']), put(g['fetch_ids']), put(g['fetch_weights']), default_id=0,
                                   default_weight=0, ncols=None)
    _equal(get(fi), g['fetch_out_ids_0'], 'fetch_single_slot ids (defaults 0)')
    _close(get(fw), g['fetch_out_weights_0'], 'fetch_single_slot weights (defaults 0)')
    fi, fw = api.fetch_single_slot(put(g['fetch_slots']), int(g['fetch_target']), put(g['fetch_ids']), put(g['fetch_weights']),
                                   default_id=int(g['fetch_default_id_1']), default_weight=float(g['fetch_default_weight_1']), ncols=None)
    _equal(get(fi), g['fetch_out_ids_1'], 'fetch_single_slot ids (defaults 10, 1)')
    _close(get(fw), g['fetch_out_weights_1'], 'fetch_single_slot weights (defaults 10, 1)')

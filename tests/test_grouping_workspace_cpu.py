"""The grouping workspace and every one-call workspace that contains it, byte for byte: host-only size functions, no GPU needed.
The tables were recorded from the build before the grouping workspace got its one layout description (csrc/grouping.hip: GroupWs); that change
retired the hierarchical-barrier experiment, whose words were the only thing allowed to move these sizes."""
import pytest

from rec_now_amd import _lib

# the `grp` and `gen` arrays of GroupMidCtl (2 x 8 x 16 unsigned words: sizeof 1152 -> 128, its 256-byte aligned slot 1280 -> 256)
RETIRED_CTL_BYTES = 1024

# B -> sizes as recorded, for n_words = 1, 2, 8
GROUP = {
    0: (272384, 276480, 301056),
    1: (272384, 276480, 301056),
    8192: (534528, 538624, 563200),
    8193: (534528, 538624, 563200),
    262143: (8659456, 8663552, 8688128),
    262144: (8661504, 8665600, 8690176),
    524288: (17050624, 17054720, 17079296),
    1048576: (34091008, 34095104, 34119680),
    1048577: (34092032, 34096128, 34120704),
    6500000: (211271936, 211276032, 211300608),
}
# B -> sizes as recorded, for the key dtypes float32, float64, int32, int64 (RECNOW_KEY_F32 = 0 ... RECNOW_KEY_I64 = 3)
PAIR = {
    0: (284416, 288512, 284416, 288512),
    1: (284416, 288512, 284416, 288512),
    8192: (1043712, 1080576, 1043712, 1080576),
    8193: (1046272, 1083136, 1046272, 1083136),
    262143: (24717056, 25769728, 24717056, 25769728),
    262144: (24719616, 25772288, 24719616, 25772288),
    524288: (49165568, 51266816, 49165568, 51266816),
    1048576: (98319616, 102518016, 98319616, 102518016),
    1048577: (98323456, 102521856, 98323456, 102521856),
    6500000: (609411840, 635415808, 609411840, 635415808),
}
LIST = {
    0: (278528, 282624, 278528, 282624),
    1: (278528, 282624, 278528, 282624),
    8192: (1233408, 1270272, 1233408, 1270272),
    8193: (1236992, 1273856, 1236992, 1273856),
    262143: (30943744, 31996416, 30943744, 31996416),
    262144: (30946816, 31999488, 30946816, 31999488),
    524288: (61618688, 63719936, 61618688, 63719936),
    1048576: (123224576, 127422976, 123224576, 127422976),
    1048577: (123229184, 127427584, 123229184, 127427584),
    6500000: (763787776, 789791744, 763787776, 789791744),
}
# the step at D = 256, S = 64, N = 2, L = 2 (B = 0 has no workspace: the constant 256, in which there is no grouping)
STEP = {
    1: (1647616, 1651712, 1647616, 1651712),
    8192: (149164288, 149201152, 149164288, 149201152),
    8193: (102614528, 102651392, 102614528, 102651392),
    262143: (2650630400, 2651683072, 2650630400, 2651683072),
    262144: (3367899904, 3368952576, 3367899904, 3368952576),
    524288: (6545430272, 6547531520, 6545430272, 6547531520),
    1048576: (12900757248, 12904955648, 12900757248, 12904955648),
    1048577: (10169755904, 10173954304, 10169755904, 10173954304),
    6500000: (62295790592, 62321794560, 62295790592, 62321794560),
}


@pytest.mark.parametrize('B', sorted(GROUP))
def test_group_segments_workspace_bytes(B):
    f = _lib.load().recnow_group_segments_workspace_bytes
    assert tuple(f(B, n) for n in (1, 2, 8)) == tuple(v - RETIRED_CTL_BYTES for v in GROUP[B])


def test_group_segments_workspace_bytes_of_invalid_inputs_is_zero():
    f = _lib.load().recnow_group_segments_workspace_bytes
    assert [f(-1, 1), f(8192, 0), f(8192, 9)] == [0, 0, 0]


@pytest.mark.parametrize('B', sorted(PAIR))
def test_one_call_workspace_bytes(B):
    lib = _lib.load()
    assert tuple(lib.recnow_pairwise_loss_workspace_bytes(B, d) for d in range(4)) == tuple(v - RETIRED_CTL_BYTES for v in PAIR[B])
    assert tuple(lib.recnow_listwise_loss_workspace_bytes(B, d) for d in range(4)) == tuple(v - RETIRED_CTL_BYTES for v in LIST[B])
    if B > 0:
        assert tuple(lib.recnow_dcn_mix_step_workspace_bytes(B, 256, 64, 2, 2, d) for d in range(4)) == tuple(v - RETIRED_CTL_BYTES for v in STEP[B])
    else:
        assert lib.recnow_dcn_mix_step_workspace_bytes(B, 256, 64, 2, 2, 0) == 256


def test_one_call_workspace_bytes_of_a_negative_batch():
    lib = _lib.load()
    assert lib.recnow_pairwise_loss_workspace_bytes(-1, 0) == 0 and lib.recnow_listwise_loss_workspace_bytes(-1, 0) == 0
    assert lib.recnow_dcn_mix_step_workspace_bytes(-1, 256, 64, 2, 2, 0) == 256

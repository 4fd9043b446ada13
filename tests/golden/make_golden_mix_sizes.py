"""Writes tests/golden/dcn_mix_sizes.npz: what the three host-only size queries of the DCN-v2 layer (recnow_dcn_mix_saved_bytes,
recnow_dcn_mix_workspace_bytes, recnow_dcn_mix_step_workspace_bytes with group dtype 0) return over a grid of shapes that reaches every branch of
the `saved` / workspace layout (csrc/dcnmix_layout.hpp): batches on and off the exact path and on both sides of the row-block rule, widths with and
without a row-block instantiation, leading dimensions 32 .. 384, L = 9 past MIX_PACK_MAX_L.  Data only; no device call is made.

The file records the layout as it was when it was written: tests/test_abi.py::test_size_queries_match_the_recorded_layout recomputes the grid with
the library under test, so run this only when a change of the layout is intended.

    python tests/golden/make_golden_mix_sizes.py
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))

BS = [1, 255, 256, 2048, 8177, 8192, 8200, 16384, 32768, 65536]
DS = [64, 256, 1024, 1152]
SS = [16, 64]
NS = [1, 2, 3, 4]
LS = [1, 2, 3, 4, 9]


def grid():
    return np.array(list(itertools.product(BS, DS, SS, NS, LS)), dtype=np.int64)


def sizes(lib, shapes):
    """(n, 3) int64: saved, workspace and step-workspace bytes of every (B, D, S, N, L) row of `shapes`."""
    return np.array([[lib.recnow_dcn_mix_saved_bytes(*s), lib.recnow_dcn_mix_workspace_bytes(*s), lib.recnow_dcn_mix_step_workspace_bytes(*s, 0)]
                     for s in shapes.tolist()], dtype=np.int64)


def main():
    from rec_now_amd import _lib
    shapes = grid()
    np.savez_compressed(os.path.join(HERE, 'dcn_mix_sizes.npz'), shapes=shapes, sizes=sizes(_lib.load(), shapes))


if __name__ == '__main__':
    main()

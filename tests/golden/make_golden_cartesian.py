"""Writes tests/golden/cartesian.npz: the expected results of the reference's own unit tests of CartesianProductLayer
(rec_now tests/layers/test_cartesian_product_layer.py), transcribed as data.  Strings are numpy 'S' arrays; a pattern that is None in the
reference is flagged in `pat_none` (its text in `pat` is then unused).

    python tests/golden/make_golden_cartesian.py
"""
import os

import numpy as np

S = lambda rows: np.array(rows, dtype='S')      # noqa: E731


def main():
    g = {}
    # the 2 x 12 product
    g['prod_in1'] = S([['A', 'B'], ['C', 'D']])
    g['prod_in2'] = S([['a', 'b', 'c'], ['d', 'e', 'f']])
    g['prod_in3'] = np.array([[1, 2], [3, 4]], dtype=np.int32)
    g['prod_plain'] = S([['A-a-1', 'A-a-2', 'A-b-1', 'A-b-2', 'A-c-1', 'A-c-2', 'B-a-1', 'B-a-2', 'B-b-1', 'B-b-2', 'B-c-1', 'B-c-2'],
                         ['C-d-3', 'C-d-4', 'C-e-3', 'C-e-4', 'C-f-3', 'C-f-4', 'D-d-3', 'D-d-4', 'D-e-3', 'D-e-4', 'D-f-3', 'D-f-4']])
    g['prod_patterns'] = S(['A', 'f', 'None'])
    g['prod_invalid'] = S([['', '', '', '', '', '', 'B-a-1', 'B-a-2', 'B-b-1', 'B-b-2', 'B-c-1', 'B-c-2'],
                           ['C-d-3', 'C-d-4', 'C-e-3', 'C-e-4', '', '', 'D-d-3', 'D-d-4', 'D-e-3', 'D-e-4', '', '']])
    # broadcast: two inputs are one row shared by the batch
    g['bcast_in1'] = S([['A', 'B']])
    g['bcast_in2'] = S('a')
    g['bcast_in3'] = np.array([[1, 2], [3, 4]], dtype=np.int32)
    g['bcast_out'] = S([['A-a-1', 'A-a-2', 'B-a-1', 'B-a-2'], ['A-a-3', 'A-a-4', 'B-a-3', 'B-a-4']])
    # digits: separator '', the texts read as numbers
    g['digits_in1'] = np.array([[[1], [2]], [[3], [4]]], dtype=np.int32)
    g['digits_in2'] = np.array([5, 6], dtype=np.int32)
    g['digits_in3'] = np.array([[7, 8], [9, 0]], dtype=np.int32)
    g['digits_out'] = np.array([[157, 158, 257, 258], [369, 360, 469, 460]], dtype=np.float32)
    # the seven pattern / result pairs on four joined strings
    g['pat_input'] = S(['A1a-na', 'B1b-', '-C1c', 'na-D1d'])
    pats = [[None, 'na'], [None, ''], ['', None], ['na', None], ['A1a|na', None], ['|na', None], ['A1a|na', '']]
    g['pat'] = S([[p or '' for p in row] for row in pats])
    g['pat_none'] = np.array([[p is None for p in row] for row in pats])
    g['pat_out'] = S([['', 'B1b-', '-C1c', 'na-D1d'], ['A1a-na', '', '-C1c', 'na-D1d'], ['A1a-na', 'B1b-', '', 'na-D1d'],
                      ['A1a-na', 'B1b-', '-C1c', ''], ['', 'B1b-', '-C1c', ''], ['A1a-na', 'B1b-', '', ''], ['', '', '-C1c', '']])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cartesian.npz'), **g)


if __name__ == '__main__':
    main()

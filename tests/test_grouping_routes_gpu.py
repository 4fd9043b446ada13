"""The grouping at the sizes where it changes route: 8192 | 8193 rows (one workgroup | one cooperative launch), 262143 | 262144 (2048 | 4096 keys per
workgroup), 1048576 | 1048577 (cooperative launch | multi-launch chain on a 256-CU device).  The invariants are those of
test_build_segments_invariants_mid_sizes (tests/_grouping_oracle.py)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _grouping_oracle as GO

pytestmark = pytest.mark.gpu


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('dtype', [np.int32, np.float32], ids=['i32', 'f32'])
@pytest.mark.parametrize('B', GO.BOUNDARY_SIZES)
def test_build_segments_invariants_at_route_boundaries(dev, B, dtype):
    from rec_now_amd.rec_block._segments import build_segments
    gs = GO.boundary_groups(B, dtype)
    GO.check_segments(build_segments([torch.from_numpy(g).to(dev) for g in gs]), gs, B)


_TILE_CHILD = r'''
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import _grouping_oracle as GO
from rec_now_amd.rec_block._segments import build_segments
h = hashlib.sha256()
for dtype in (np.int32, np.float32):
    seg = build_segments([torch.from_numpy(g).to('cuda:0') for g in GO.boundary_groups(20000, dtype)])
    for a in GO.segment_arrays(seg, 20000):
        h.update(np.ascontiguousarray(a).tobytes())
print('DIGEST', h.hexdigest())
'''


def test_group_tile_4096_gives_the_default_arrays(dev):
    """RECNOW_GROUP_TILE=4096 (read once per process: a child) moves 20 000 rows from ten workgroups of 2048 keys to five of 4096: same arrays."""
    from rec_now_amd.rec_block._segments import build_segments
    here = []
    for dtype in (np.int32, np.float32):
        gs = GO.boundary_groups(20000, dtype)
        seg = build_segments([torch.from_numpy(g).to(dev) for g in gs])
        GO.check_segments(seg, gs, 20000)
        here += list(GO.segment_arrays(seg, 20000))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['RECNOW_GROUP_TILE'] = '4096'
    out = subprocess.run([sys.executable, '-c', _TILE_CHILD % {'root': root}], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert [l for l in out.stdout.splitlines() if l.startswith('DIGEST')][-1] == 'DIGEST ' + _digest(here)

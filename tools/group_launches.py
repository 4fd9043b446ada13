"""Which kernels a batch's grouping launches, consumer by consumer: one call of the one-call `pairwise_loss` and `listwise_loss_from_batch` per
(rows, id type) cell of tools/group_bits.py and one `DCNMixPairwiseStep.run()` per step size, for a rocprofv3 kernel trace; and the reader of that trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/group_launches.py
    python tools/group_launches.py DIR/*/*_kernel_trace.csv       -> the library's launches in start order: name, grid, workgroup

Two builds that take the same routes print the same list.  GPU only, diagnostic."""
import csv, os, sys

if len(sys.argv) > 1:
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r['Start_Timestamp']))
    for r in rows:
        if 'at::native' in r['Kernel_Name']:        # torch's own element-wise kernels (input preparation)
            continue
        print('%-72s grid %8s  workgroup %5s' % (r['Kernel_Name'].replace('void ', '').split('(')[0][:72], r['Grid_Size_X'] if 'Grid_Size_X' in r else r['Grid_Size'],
                                                 r['Workgroup_Size_X'] if 'Workgroup_Size_X' in r else r['Workgroup_Size']))
    sys.exit(0)

import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
from rec_now_amd.rec_block.listwise_loss_from_batch import listwise_loss_from_batch
from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
from rec_now_amd.step import DCNMixPairwiseStep
from test_step_gpu import _model

dev = torch.device('cuda:0')
for B in (8192, 8193, 20000):
    rng = np.random.default_rng(B)
    y = torch.from_numpy((rng.random(B) < 0.3).astype(np.float32)).to(dev)
    s = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev)
    ids = rng.integers(0, 400, B)
    for dtype in (np.float32, np.int32, np.int64, np.float64):
        gd = torch.from_numpy(ids.astype(dtype)).to(dev)
        pairwise_loss(s, y, gd)
        listwise_loss_from_batch(gd, y, s)
        torch.cuda.synchronize()
for B in (8192, 16384):
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, 256, 64, 2, 2, 77)
    DCNMixPairwiseStep(cross, head, xd, yd, gd).run()
    torch.cuda.synchronize()

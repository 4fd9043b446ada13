"""Bit-level fingerprint of the grouping and of everything that starts from it in one library call.  SHA-256 digests of
  * `order`, `seg_id`, `seg_first[:n_seg + 1]`, `super_id`, `n_seg` of `build_segments` for every case of test_build_segments_invariants_mid_sizes, for
    one int32 and one float32 id tensor at the sizes where the grouping changes route (tests/_grouping_oracle.py: BOUNDARY_SIZES), and for two group
    tensors at 8000 rows (several key words leave the one-workgroup route);
  * loss and gradient of the one-call `pairwise_loss` and `listwise_loss_from_batch` at 8192, 8193 and 20000 rows with float32 (NaN, +-inf, -0.0
    among them), int32, int64 and float64 ids;
  * scores, loss, pair count and d loss / d x of `DCNMixPairwiseStep` at 8192 and 16384 rows, run twice, in one child process each for
    RECNOW_STEP_FRONT=0 and 1 (the switch is read once per process).
Two builds of the library compute the same bits exactly when their files are byte-identical; GPU only, diagnostic.

    RECNOW_LIB_PATH=/path/to/librecnow_hip.so python tools/group_bits.py OUT.json      (one build per process; the package is the one beside tools/)
"""
import hashlib, json, os, subprocess, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
import _grouping_oracle as GO
from rec_now_amd import _lib
from rec_now_amd.rec_block._segments import build_segments

dev = torch.device('cuda:0')
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()      # noqa: E731
LOSS_SIZES = (8192, 8193, 20000)
STEP_SIZES = (8192, 16384)


def loss_ids(B, kind):
    rng = np.random.default_rng(B + len(kind))
    g = rng.integers(0, 400, B)
    if kind in ('f32', 'f64'):
        g = g.astype(np.float32 if kind == 'f32' else np.float64)
        g[::211] = np.nan
        g[3::307] = np.inf
        g[5::401] = -np.inf
        g[g == 0][::2] = -0.0
        g[7::97] = -0.0
        return g
    return (g - 50).astype(np.int32) if kind == 'i32' else (g.astype(np.int64) - 50) * (2 ** 33 + 1)


def step_entries():
    from test_step_gpu import _model
    from rec_now_amd.step import DCNMixPairwiseStep
    out = {}
    for B in STEP_SIZES:
        x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, 256, 64, 2, 2, 77)
        step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
        for _ in range(2):
            loss, n_pair = step.run()
        torch.cuda.synchronize()
        out['step/front%s-%d' % (os.environ['RECNOW_STEP_FRONT'], B)] = {
            'scores': sha(step.scores.detach().cpu().numpy()), 'loss': sha(loss.detach().cpu().numpy()), 'n_pair': int(n_pair.item()),
            'dx': sha(step.dx.detach().cpu().numpy())}
    return out


if len(sys.argv) > 2 and sys.argv[2] == '--step-child':
    with open(sys.argv[1], 'w') as f:
        json.dump(step_entries(), f)
    sys.exit(0)

out = {}


def segments_entry(name, gs, B):
    seg = build_segments([torch.from_numpy(g).to(dev) for g in gs])
    order, seg_id, seg_first, super_id, n_seg = GO.segment_arrays(seg, B)
    out['segments/' + name] = {'order': sha(order), 'seg_id': sha(seg_id), 'seg_first': sha(seg_first), 'super_id': sha(super_id),
                               'n_seg': [int(v) for v in n_seg]}


for B, kind in GO.MID_CASES:
    segments_entry('%d-%s' % (B, kind), GO.mid_size_groups(B, kind), B)
for B in GO.BOUNDARY_SIZES:
    for name, dtype in (('i32', np.int32), ('f32', np.float32)):
        segments_entry('boundary-%d-%s' % (B, name), GO.boundary_groups(B, dtype), B)
segments_entry('8000-two-tensors', [GO.mid_size_groups(8000, 'int_img')[0], GO.mid_size_groups(8000, 'frac')[0]], 8000)

from rec_now_amd.rec_block.listwise_loss_from_batch import listwise_loss_from_batch
from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
for B in LOSS_SIZES:
    rng = np.random.default_rng(B)
    y = torch.from_numpy(rng.integers(0, 3, B).astype(np.float32)).to(dev)
    s0 = rng.normal(size=B).astype(np.float32)
    for kind in ('f32', 'i32', 'i64', 'f64'):
        gd = torch.from_numpy(loss_ids(B, kind)).to(dev)
        sd = torch.from_numpy(s0).to(dev).requires_grad_(True)
        loss, n_pair = pairwise_loss(sd, y, gd, return_num_pair=True)
        loss.backward()
        out['pairwise/%d-%s' % (B, kind)] = {'loss': sha(loss.detach().cpu().numpy()), 'n_pair': int(n_pair.item()), 'grad': sha(sd.grad.cpu().numpy())}
        sd = torch.from_numpy(s0).to(dev).requires_grad_(True)
        loss, n_list = listwise_loss_from_batch(gd, (y > 0).float(), sd, return_num_list=True)
        loss.backward()
        out['listwise/%d-%s' % (B, kind)] = {'loss': sha(loss.detach().cpu().numpy()), 'n_list': int(n_list.item()), 'grad': sha(sd.grad.cpu().numpy())}

for front in ('0', '1'):
    part = sys.argv[1] + '.front' + front
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['RECNOW_STEP_FRONT'] = front
    subprocess.run([sys.executable, os.path.abspath(__file__), part, '--step-child'], check=True, env=env, timeout=300)
    with open(part) as f:
        out.update(json.load(f))
    os.remove(part)

with open(sys.argv[1], 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print('group_bits: %d entries from %s -> %s' % (len(out), _lib.LIB_PATH, sys.argv[1]))

"""Bit-level fingerprint of the pair walks: every case of tests/test_pair_walk_routes_gpu.CASES through `pairwise_loss` (loss, pair count and
gradient bytes), `cnt_row` of recnow_pair_count and recnow_pair_table_count with and without the wrong-order rule, and every output of
recnow_pair_lambda_terms, on the three route layouts of tests/_pair_lists_oracle.py; then, on one layout, the host routes those cases do not
reach (`pairwise_loss_fused(..., segments=)` at power 0 as a mean and as a sum, a list of two group tensors at power 0, int64 ids at power
-0.5) and every output of the public `ndcg_rank_terms`, `in_batch_ndcg`, `auc_terms` and `in_batch_gauc`.  Writes one JSON of SHA-256 digests.
Two builds of the library, or two versions of the Python package on one build, compute the same bits exactly when their files are
byte-identical; GPU only, diagnostic.

    RECNOW_LIB_PATH=/path/to/librecnow_hip.so python tools/pair_bits.py OUT.json      (one build per process; the package is the one beside tools/)
"""
import hashlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import _pair_lists_oracle as O
import test_pair_walk_routes_gpu as T
from rec_now_amd import _lib
from rec_now_amd.rec_block import ndcg as N

dev = torch.device('cuda:0')
M = T._mod()
M.pair_indices = None                            # the general route would fail loudly
P, st = _lib.ptr, _lib.stream()
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()      # noqa: E731
out = {}

for case in T.CASES:
    loss, n_pair, grad = T._run(M, dev, *case)
    out['loss/' + T._case_id(case)] = {'loss': sha(np.float32(loss)), 'n_pair': int(n_pair), 'grad': sha(grad)}

for name in T.NAMES:
    g, s, y, mask = O.layout(name)
    seg = M.group_rows(T._t(g).to(dev))
    B = seg.B
    sd, yd, m8 = T._t(s).to(dev), T._t(y).to(dev), T._t(mask).to(dev).to(torch.uint8).contiguous()
    seg_args = (P(seg.order), P(seg.seg_id), P(seg.seg_first))
    ws = _lib.workspace(_lib.load().recnow_pairwise_workspace_bytes(B), dev)
    vals, w = M.LabelPairWeightTable(O.LEVELS, O.w_sym).on_device(dev)
    for wrong in (False, True):
        for rule in ('default', 'sym'):
            cnt_row = torch.full((B,), -1, dtype=torch.int32, device=dev)
            cnt_super = torch.empty(B, dtype=torch.int64, device=dev)
            n_pair = torch.full((1,), -1, dtype=torch.int64, device=dev)
            if rule == 'sym':
                _lib.call('recnow_pair_table_count', P(sd), P(yd), P(m8), *seg_args, P(seg.super_id), B, T.FLAG_WRONG_ORDER if wrong else 0,
                          P(vals), 4, P(w), P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
            else:
                _lib.call('recnow_pair_count', P(sd), P(yd), P(m8), *seg_args, P(seg.super_id), B,
                          T.FLAG_LABEL_GT | (T.FLAG_WRONG_ORDER if wrong else 0), P(cnt_row), P(cnt_super), P(n_pair), P(ws), ws.numel(), st)
            out['count/%s-%s-%s' % (name, rule, 'wrong' if wrong else 'all')] = {'cnt_row': sha(cnt_row.cpu().numpy()), 'n_pair': int(n_pair.item())}
    lws = N.lambda_workspace(B, dev)
    for gain, topn in (('exp2', 0), ('linear', 5), ('exp2', T.FAR)):
        bufs = {'rank': torch.full((B,), -7, dtype=torch.int32, device=dev), 'ndcg_mean': torch.full((1,), -1.0, device=dev),
                'n_lists': torch.full((1,), -1, dtype=torch.int64, device=dev)}
        bufs.update({k: torch.full((B,), -1.0, device=dev) for k in ('discount', 'gain', 'inv_idcg')})
        bufs.update({k: torch.full((B,), -1.0, dtype=torch.float64, device=dev) for k in ('list_dcg', 'list_idcg')})
        _lib.call('recnow_pair_lambda_terms', P(sd), P(yd), P(m8), *seg_args, B, 0, {'exp2': 0, 'linear': 1}[gain], topn,
                  *[P(bufs[k]) for k in ('rank', 'discount', 'gain', 'inv_idcg', 'list_dcg', 'list_idcg', 'ndcg_mean', 'n_lists')], P(lws), lws.numel(), st)
        out['terms/%s-%s-%d' % (name, gain, topn)] = {k: sha(v.cpu().numpy()) for k, v in bufs.items()}

# the host routes the cases above do not reach, and the public metric entries, on one layout
from rec_now_amd.rec_block import auc as A
g, s, y, mask = O.layout('chain')
gd, yd, md = T._t(g).to(dev), T._t(y).to(dev), T._t(mask).to(dev)
routes = {'fused-segments-mean': lambda sd: M.pairwise_loss_fused(sd, yd, None, mask=md, reduce_mean=True, segments=M.group_rows(gd)),
          'fused-segments-sum': lambda sd: M.pairwise_loss_fused(sd, yd, None, mask=md, reduce_mean=False, segments=M.group_rows(gd)),
          'two-tensors-pow0': lambda sd: M.pairwise_loss(sd, yd, [gd, T._t(O.second_groups(g.size)).to(dev)], return_num_pair=True, mask=md),
          'int64-ids-pow-0.5': lambda sd: M.pairwise_loss(sd, yd, gd.to(torch.int64), return_num_pair=True, click_occurance_power=-0.5, mask=md)}
for name, fn in routes.items():
    sd = T._t(s).to(dev).requires_grad_(True)
    loss, n_pair = fn(sd)
    loss.backward()
    out['host/' + name] = {'loss': sha(loss.detach().cpu().numpy()), 'n_pair': int(n_pair.item()), 'grad': sha(sd.grad.cpu().numpy())}
sd = T._t(s).to(dev)
metrics = {'ndcg_rank_terms': N.ndcg_rank_terms(sd, yd, gd, mask=md, topn=5), 'in_batch_ndcg': N.in_batch_ndcg(sd, yd, gd, mask=md),
           'auc_terms': A.auc_terms(sd, yd, gd, mask=md), 'in_batch_gauc': A.in_batch_gauc(sd, yd, gd, mask=md)}
n_seg = M.group_rows(gd).num_segments()
for name, res in metrics.items():
    fields = getattr(res, '_fields', None) or ['%d' % i for i in range(len(res))]
    out['metric/' + name] = {k: sha((v[:n_seg] if k.startswith('list_') else v).cpu().numpy()) for k, v in zip(fields, res)}

with open(sys.argv[1], 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print('pair_bits: %d entries from %s -> %s' % (len(out), _lib.LIB_PATH, sys.argv[1]))

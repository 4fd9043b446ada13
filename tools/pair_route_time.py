"""GPU time, to four decimals, of the pair-loss routes that tools/layer_bench.py prints to three or does not run: the plain family's segments route
(click_occurance_power -0.5: recnow_pair_count + recnow_pair_bpr_fwdbwd) with and without only_use_wrong_order_pair at B 65 536 on 1024 uniform
groups and on Zipf 1.2 group sizes capped at 2048, and the table BPR / hinge / margin-logistic / NDCG routes at the shape of pair_table().  The step
is replayed from a HIP graph, 50 repetitions after 10 warm-ups, every route twice in the process (layer_bench.py's method).  GPU only; diagnostic.

    [RECNOW_LIB_PATH=/path/to/librecnow_hip.so] python tools/pair_route_time.py
"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
dev = torch.device('cuda:0')

def timeit(fn, n=50):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n

def graph_time(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return timeit(g.replay)

def zipf_groups(rng, B, a=1.2, cap=2048):
    sizes = []
    while sum(sizes) < B:
        sizes.append(int(min(rng.zipf(a), cap, B - sum(sizes))))
    g = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(g)
    return g.astype(np.float32)

B = 65536
for tag in ('uniform1024', 'zipf'):
    rng = np.random.default_rng(2)
    g = torch.from_numpy(zipf_groups(rng, B) if tag == 'zipf' else rng.integers(0, 1024, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)
    for wrong in (False, True):
        def step():
            s.grad = None
            pairwise_loss(s, y, g, only_use_wrong_order_pair=wrong, click_occurance_power=-0.5).backward()
        for run in (1, 2):
            print('run %d  plain segments route %s wrong=%s : GPU %.4f ms (graph replay)' % (run, tag, wrong, graph_time(step)), flush=True)

# the routes of tools/layer_bench.py pair_table / pair_kind / pair_lambda once more, to four decimals
from rec_now_amd.rec_block.pairwise_loss_from_batch import LabelPairWeightTable, bpr_loss_func, hinge_loss_func, margin_bpr_loss_func
from rec_now_amd.rec_block.ndcg import NDCGLambdaWeight
rng = np.random.default_rng(2)
g = torch.from_numpy(rng.integers(0, 1024, B).astype(np.float32)).to(dev)
y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
s = torch.randn(B, device=dev, requires_grad=True)
table = LabelPairWeightTable([0.0, 1.0, 2.0, 3.0], lambda a, b: (a - b).abs() + 0.5)
lam = NDCGLambdaWeight()
for tag, kw in (('table BPR', {}), ('table hinge', {'pairloss_func': hinge_loss_func}), ('table margin_bpr', {'pairloss_func': margin_bpr_loss_func}),
                ('table BPR + lambda', {'pairloss_func': bpr_loss_func, 'lambda_weight': lam}), ('table hinge + lambda', {'pairloss_func': hinge_loss_func, 'lambda_weight': lam})):
    def step():
        s.grad = None
        pairwise_loss(s, y, g, label_pair_to_weight_func=table, **kw).backward()
    for run in (1, 2):
        print('run %d  plain segments route %s wrong=- : GPU %.4f ms (graph replay)' % (run, tag.replace(' ', '_'), graph_time(step)), flush=True)

"""Per-row measurements of the other hot-path kernels at BASELINE config sizes (1x MI355X), fwd+bwd, inputs resident.
Reports the figure each kernel's roofline is priced in: HBM GB/s for FM / DCN-v1 / MoE mix,
rows/s and pairs/s for the ranking losses, TFLOP/s for CIN / MMoE / PLE.   usage: python tools/layer_bench.py [reps] [fm,dcn,pair,pair_table,pair_kind,pair_lambda,pair_auc,pair_auc_sort,list,listmle,approx_ndcg,cin,ple,star,stacked,gnn,ipnn,senet,attn,din,focal,embed,hash,cross,slot,tensor_util,can,bilinear,autoint,afm,in_batch_softmax,in_batch_softmax_extra,in_batch_ranks,in_batch_top_k,attention_softmax]"""
import os
import sys

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')      # see bench.py: ROCm 7.0 graph packet capture + eager launches of the same kernels

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dev = torch.device('cuda:0')
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def timeit(fn, n=reps, warm=10):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms


def timeit_graph(fn, n=reps):
    """The same step replayed from a captured HIP graph: no Python or launch overhead between kernels, i.e. the GPU time of
    the step.  Returns None when the step cannot be captured (data-dependent host work)."""
    if os.environ.get('RECNOW_LB_NOGRAPH') == '1':      # under rocprofv3: the eager launches are what gets traced
        return None
    try:
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
        return timeit(g.replay, n)
    except Exception as e:          # noqa: BLE001
        torch.cuda.synchronize()
        print('   (graph capture not possible: %s)' % repr(e)[:120])
        return None


def fm():
    from rec_now_amd.layers.fm_layer import FMLayer
    B, F, D = 131072, 64, 16                # config 4 global batch
    xs = [torch.randn(B, D, device=dev, requires_grad=True) for _ in range(F)]
    layer = FMLayer()
    gy = torch.randn(B, 1, device=dev)

    def step():
        for x in xs:
            x.grad = None
        layer(xs).backward(gy)
    ms = timeit(step)
    print('FMLayer fwd+bwd   B=%d F=%d D=%d : %.3f ms  %.0f GB/s algorithmic (12*B*F*D bytes)  %.1f M samples/s'
          % (B, F, D, ms, 12.0 * B * F * D / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (no host time between the 2 kernels and autograd\'s 64 leaves): %.3f ms  %.0f GB/s'
              % (mg, 12.0 * B * F * D / mg / 1e6))


def dcn():
    from rec_now_amd.layers.dcn_layer import DCNLayer
    B, D, L = 65536, 1024, 3
    x = torch.randn(B, D, device=dev, requires_grad=True)
    layer = DCNLayer(L)
    gy = torch.randn(B, D, device=dev)
    layer(x)

    def step():
        x.grad = None
        layer(x).backward(gy)
    ms = timeit(step)
    print('DCNLayer fwd+bwd  B=%d D=%d L=%d : %.3f ms  %.0f GB/s algorithmic (20*B*D bytes: x,y | x,dy,dx)  %.1f M samples/s'
          % (B, D, L, ms, 20.0 * B * D / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.0f GB/s' % (mg, 20.0 * B * D / mg / 1e6))


def zipf_groups(rng, B, a=1.2, cap=2048):
    """SURVEY 8d config 2, skewed variant: group sizes ~ Zipf(a) capped at `cap`, rows shuffled."""
    sizes = []
    while sum(sizes) < B:
        sizes.append(int(min(rng.zipf(a), cap, B - sum(sizes))))
    g = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(g)
    return g.astype(np.float32), len(sizes)


def pairwise(B, G, tag):
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    rng = np.random.default_rng(2)
    if G == 0:
        gn, G = zipf_groups(rng, B)
        g = torch.from_numpy(gn).to(dev)
    else:
        g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.random(B) < 0.25).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)
    npair = [0.0]

    def step():
        s.grad = None
        loss, n = pairwise_loss(s, y, g, return_num_pair=True)
        loss.backward()
        npair[0] = n
    ms = timeit(step)
    P = float(npair[0].item())
    print('pairwise_loss %s B=%d groups=%d pairs=%d : %.3f ms  %.1f M rows/s  %.1f M pairs/s' % (tag, B, G, P, ms, B / ms / 1e3, P / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.1f M rows/s' % (mg, B / mg / 1e3))


def pair_table():
    """pairwise_loss with per-label-pair weights at config 3's shape (B = 65 536, 1024 groups, four label levels, weight |a - b| + 0.5: both
    directions and tied labels are pairs): the fused table route, the general route with the same table (handed over as a plain callable) and
    the default fused loss without a table as the yardstick -- wall time per step, and GPU time (the step replayed from a HIP graph) where the
    route can be captured."""
    from rec_now_amd.rec_block.pairwise_loss_from_batch import LabelPairWeightTable, pairwise_loss
    B, G = 65536, 1024
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)
    table = LabelPairWeightTable([0.0, 1.0, 2.0, 3.0], lambda a, b: (a - b).abs() + 0.5)
    rows = (('table route', {'label_pair_to_weight_func': table}),
            ('general route, same table', {'label_pair_to_weight_func': lambda a, b, **k: table(a, b)}),
            ('default fused loss, no table', {}))
    res = {}
    for tag, kw in rows:
        npair = [None]

        def step():
            s.grad = None
            loss, n = pairwise_loss(s, y, g, return_num_pair=True, **kw)
            loss.backward()
            npair[0] = n
        ms = timeit(step)
        mg = timeit_graph(step)
        res[tag] = (ms, mg)
        print('pairwise_loss %s B=%d groups=%d pairs=%d : wall %.3f ms per fwd+bwd, GPU %s' % (
            tag, B, G, float(npair[0].item()), ms, ('%.3f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisations: no capture)'))
    t, ge, d = res['table route'], res['general route, same table'], res['default fused loss, no table']
    print('   wall: general / table = %.1fx, table / default = %.2fx' % (ge[0] / t[0], t[0] / d[0]))
    if t[1] and d[1]:
        print('   GPU: table / default = %.2fx; general route wall / table GPU = %.1fx' % (t[1] / d[1], ge[0] / t[1]))


def pair_kind():
    """pairwise_loss with a pair loss other than BPR at the shape of pair_table() (B = 65 536, 1024 groups, four label levels, the table
    |a - b| + 0.5): hinge_loss_func on the fused route, the same function inside a lambda (the general route: pairs materialised, one host
    synchronisation -- not capturable, so wall time only), margin_bpr_loss_func on the fused route and the BPR table route as the yardstick.
    Wall time per forward + backward and GPU time (the step replayed from a HIP graph); the four routes are measured in turn, twice, so the
    spread between the two passes stands beside every ratio."""
    from rec_now_amd.rec_block.pairwise_loss_from_batch import (LabelPairWeightTable, hinge_loss_func, margin_bpr_loss_func, pairwise_loss)
    B, G = 65536, 1024
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)
    table = LabelPairWeightTable([0.0, 1.0, 2.0, 3.0], lambda a, b: (a - b).abs() + 0.5)
    rows = (('hinge fused', {'pairloss_func': hinge_loss_func}, True),
            ('hinge in a lambda (general route)', {'pairloss_func': lambda p, n, w: hinge_loss_func(p, n, w)}, False),
            ('margin_bpr fused', {'pairloss_func': margin_bpr_loss_func}, True),
            ('BPR table route', {}, True))
    res = {tag: [] for tag, _, _ in rows}
    for run in (1, 2):
        for tag, kw, capture in rows:
            npair = [None]

            def step():
                s.grad = None
                loss, n = pairwise_loss(s, y, g, return_num_pair=True, label_pair_to_weight_func=table, **kw)
                loss.backward()
                npair[0] = n
            ms = timeit(step)
            mg = timeit_graph(step) if capture else None
            res[tag].append((ms, mg))
            print('run %d  pairwise_loss %s B=%d groups=%d pairs=%d : wall %.3f ms per fwd+bwd, GPU %s' % (
                run, tag, B, G, float(npair[0].item()), ms,
                ('%.3f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisation: no capture)'))
    h, lam, mb, t = (res[tag] for tag, _, _ in rows)
    for run in (0, 1):
        line = '   run %d  wall: general / hinge fused = %.1fx' % (run + 1, lam[run][0] / h[run][0])
        if h[run][1] and mb[run][1] and t[run][1]:
            line += ';  GPU: hinge / table = %.2fx, margin_bpr / table = %.2fx' % (h[run][1] / t[run][1], mb[run][1] / t[run][1])
        print(line)
    print('   spread between the two runs, wall: hinge fused %.3f ms, general %.3f ms' % (abs(h[0][0] - h[1][0]), abs(lam[0][0] - lam[1][0])))
    if all(r[1] for r in h + mb + t):
        print('   spread between the two runs, GPU: hinge fused %.4f ms, margin_bpr fused %.4f ms, BPR table route %.4f ms'
              % (abs(h[0][1] - h[1][1]), abs(mb[0][1] - mb[1][1]), abs(t[0][1] - t[1][1])))


def pair_lambda():
    """pairwise_loss with the NDCG (LambdaRank) pair weight at the shape of pair_kind() (B = 65 536, 1024 groups, four label levels, the table
    |a - b| + 0.5): BPR and hinge_loss_func with `lambda_weight=NDCGLambdaWeight()` on the fused route (count, rank pre-pass, lambda walk), the
    same two losses without the weight (the existing table routes: the yardstick), and BPR with the weight inside a lambda (the general route:
    pairs materialised, one host synchronisation -- not capturable, so wall time only).  Wall time per forward + backward and GPU time (the
    step replayed from a HIP graph); the routes are measured in turn, twice, so the spread between the two passes stands beside every ratio."""
    from rec_now_amd.rec_block.ndcg import NDCGLambdaWeight
    from rec_now_amd.rec_block.pairwise_loss_from_batch import (LabelPairWeightTable, bpr_loss_func, hinge_loss_func, pairwise_loss)
    B, G = 65536, 1024
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)
    table = LabelPairWeightTable([0.0, 1.0, 2.0, 3.0], lambda a, b: (a - b).abs() + 0.5)
    lam = NDCGLambdaWeight()
    rows = (('BPR + lambda fused', {'lambda_weight': lam}, True),
            ('hinge + lambda fused', {'pairloss_func': hinge_loss_func, 'lambda_weight': lam}, True),
            ('BPR table route, no lambda', {}, True),
            ('hinge fused, no lambda', {'pairloss_func': hinge_loss_func}, True),
            ('BPR + lambda in a lambda (general route)', {'pairloss_func': lambda p, n, w: bpr_loss_func(p, n, w), 'lambda_weight': lam}, False))
    res = {tag: [] for tag, _, _ in rows}
    for run in (1, 2):
        for tag, kw, capture in rows:
            npair = [None]

            def step():
                s.grad = None
                loss, n = pairwise_loss(s, y, g, return_num_pair=True, label_pair_to_weight_func=table, **kw)
                loss.backward()
                npair[0] = n
            ms = timeit(step)
            mg = timeit_graph(step) if capture else None
            res[tag].append((ms, mg))
            print('run %d  pairwise_loss %s B=%d groups=%d pairs=%d : wall %.3f ms per fwd+bwd, GPU %s' % (
                run, tag, B, G, float(npair[0].item()), ms,
                ('%.3f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisation: no capture)'))
    bl, hl, b0, h0, ge = (res[tag] for tag, _, _ in rows)
    for run in (0, 1):
        line = '   run %d  wall: BPR lambda / BPR = %.2fx, hinge lambda / hinge = %.2fx, general / BPR lambda fused = %.1fx' % (
            run + 1, bl[run][0] / b0[run][0], hl[run][0] / h0[run][0], ge[run][0] / bl[run][0])
        if all(r[run][1] for r in (bl, hl, b0, h0)):
            line += ';  GPU: BPR lambda / BPR = %.2fx, hinge lambda / hinge = %.2fx' % (bl[run][1] / b0[run][1], hl[run][1] / h0[run][1])
        print(line)
    print('   spread between the two runs, wall: BPR lambda fused %.3f ms, general %.3f ms' % (abs(bl[0][0] - bl[1][0]), abs(ge[0][0] - ge[1][0])))
    if all(r[1] for r in bl + hl + b0 + h0):
        print('   spread between the two runs, GPU: BPR lambda %.4f ms, hinge lambda %.4f ms, BPR table route %.4f ms, hinge fused %.4f ms'
              % (abs(bl[0][1] - bl[1][1]), abs(hl[0][1] - hl[1][1]), abs(b0[0][1] - b0[1][1]), abs(h0[0][1] - h0[1][1])))


def pair_auc():
    """in_batch_gauc at the shape of pair_lambda() (B = 65 536, 1024 groups, four label levels): the fused metric under the graded rule and
    under the binary rule (pos_neg_th = 1.5), in_batch_ndcg on the same batch as the yardstick (the same single compare-only traversal plus
    the same kind of segment and metric kernels), and the same metric from pair_indices plus torch ops (pairs materialised, one host
    synchronisation -- not capturable, so wall time only).  Wall time per call and GPU time (the call replayed from a HIP graph); the routes
    are measured in turn, twice, so the spread between the two passes stands beside every ratio."""
    from rec_now_amd.rec_block.auc import in_batch_gauc
    from rec_now_amd.rec_block.ndcg import in_batch_ndcg
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pair_indices
    B, G = 65536, 1024
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev)
    out = [None]

    def host_route():
        """impressions-weighted GAUC under the graded rule from the materialised pair list"""
        pos, neg = pair_indices(s, y, g)
        pos, neg = pos.long(), neg.long()
        _, lid = torch.unique(g, return_inverse=True)
        n_list = int(lid.max().item()) + 1
        sp, sn, lp = s[pos], s[neg], lid[pos]
        N = torch.bincount(lp, minlength=n_list).double()
        C = torch.bincount(lp, weights=(sp > sn).double(), minlength=n_list)
        T = torch.bincount(lp, weights=(sp == sn).double(), minlength=n_list)
        R = torch.bincount(lid, minlength=n_list).double()
        ok = N > 0
        out[0] = ((R[ok] * (2 * C[ok] + T[ok]) / (2 * N[ok])).sum() / R[ok].sum()).float()

    def fused(**kw):
        def step():
            out[0] = in_batch_gauc(s, y, g, **kw).auc
        return step

    def ndcg():
        out[0] = in_batch_ndcg(s, y, g)[0]
    rows = (('in_batch_gauc graded', fused(), True), ('in_batch_gauc pos_neg_th=1.5', fused(pos_neg_th=1.5), True),
            ('in_batch_ndcg (yardstick)', ndcg, True), ('GAUC graded from pair_indices + torch ops (host route)', host_route, False))
    res = {tag: [] for tag, _, _ in rows}
    for run in (1, 2):
        for tag, step, capture in rows:
            ms = timeit(step)
            value = float(out[0].item())
            mg = timeit_graph(step) if capture else None
            res[tag].append((ms, mg))
            print('run %d  %s B=%d groups=%d value=%.7f : wall %.3f ms per call, GPU %s' % (
                run, tag, B, G, value, ms, ('%.4f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisation: no capture)'))
    gr, bi, nd, ho = (res[tag] for tag, _, _ in rows)
    for run in (0, 1):
        line = '   run %d  wall: host route / gauc graded = %.1fx, gauc graded / ndcg = %.2fx, gauc binary / ndcg = %.2fx' % (
            run + 1, ho[run][0] / gr[run][0], gr[run][0] / nd[run][0], bi[run][0] / nd[run][0])
        if all(r[run][1] for r in (gr, bi, nd)):
            line += ';  GPU: gauc graded / ndcg = %.2fx, gauc binary / ndcg = %.2fx, host route wall / gauc graded GPU = %.1fx' % (
                gr[run][1] / nd[run][1], bi[run][1] / nd[run][1], ho[run][0] / gr[run][1])
        print(line)
    print('   spread between the two runs, wall: gauc graded %.3f ms, gauc binary %.3f ms, ndcg %.3f ms, host route %.3f ms'
          % tuple(abs(r[0][0] - r[1][0]) for r in (gr, bi, nd, ho)))
    if all(r[1] for r in gr + bi + nd):
        print('   spread between the two runs, GPU: gauc graded %.4f ms, gauc binary %.4f ms, ndcg %.4f ms'
              % tuple(abs(r[0][1] - r[1][1]) for r in (gr, bi, nd)))


def pair_auc_sort():
    """The two routes of the in-batch GAUC / AUC, walk against sort (rec_block/auc.py, route=): the shape of pair_auc() (B = 65 536, 1024 groups,
    four label levels) under the graded and the binary rule; ONE list (in_batch_auc, graded rule, four levels) at every power of two from 1024
    to 262 144 rows, which is the sweep `AUC_SORT_FROM` is set from; one list of 1 048 576 rows on the sort route alone (the walk would look at
    1e12 candidates).  Wall time per call and GPU time (the call replayed from a HIP graph); the routes are measured in turn, twice, so the
    spread between the two passes stands beside every ratio.  The walk gets few repetitions on the long lists."""
    from rec_now_amd.rec_block.auc import in_batch_auc, in_batch_gauc
    rng = np.random.default_rng(2)
    out = [None]

    def measure(tag, cases, n):
        res = {name: [] for name, _ in cases}
        for run in (1, 2):
            for name, step in cases:
                ms = timeit(step, n=n, warm=2)
                value = float(out[0].item())
                mg = timeit_graph(step, n=n)
                res[name].append((ms, mg))
                print('run %d  %s %s value=%.7f : wall %.3f ms per call, GPU %s' % (
                    run, tag, name, value, ms, ('%.4f ms (graph replay)' % mg) if mg else 'not measured (no capture)'))
        if 'walk' in res and 'sort' in res:
            w, so = res['walk'], res['sort']
            line = '   %s  walk / sort, wall: %.2fx, %.2fx' % (tag, w[0][0] / so[0][0], w[1][0] / so[1][0])
            if all(r[1] for r in w + so):
                line += ';  GPU: %.2fx, %.2fx;  spread between the two runs, GPU: walk %.4f ms, sort %.4f ms' % (
                    w[0][1] / so[0][1], w[1][1] / so[1][1], abs(w[0][1] - w[1][1]), abs(so[0][1] - so[1][1]))
            print(line)
        return res

    B, G = 65536, 1024
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev)

    def gauc(route, **kw):
        def step():
            out[0] = in_batch_gauc(s, y, g, route=route, **kw).auc
        return step
    measure('in_batch_gauc graded B=%d groups=%d' % (B, G), (('walk', gauc('walk')), ('sort', gauc('sort'))), reps)
    measure('in_batch_gauc pos_neg_th=1.5 B=%d groups=%d' % (B, G), (('walk', gauc('walk', pos_neg_th=1.5)), ('sort', gauc('sort', pos_neg_th=1.5))), reps)

    def auc(route, s1, y1):
        def step():
            out[0] = in_batch_auc(s1, y1, route=route).auc
        return step
    for B1 in [1 << k for k in range(10, 19)] + [1 << 20]:
        y1 = torch.from_numpy(rng.integers(0, 4, B1).astype(np.float32)).to(dev)
        s1 = torch.randn(B1, device=dev)
        cases = (('walk', auc('walk', s1, y1)), ('sort', auc('sort', s1, y1))) if B1 <= 262144 else (('sort', auc('sort', s1, y1)),)
        measure('in_batch_auc graded, one list of B=%d' % B1, cases, reps if B1 <= 16384 else max(2, min(reps, (1 << 21) // B1)))


def listwise():
    from rec_now_amd.rec_block.listwise_loss_from_batch import listwise_loss_from_batch
    B, G = 262144, 4096
    rng = np.random.default_rng(5)
    g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.random(B) < 0.25).astype(np.float32)).to(dev)
    s = torch.randn(B, device=dev, requires_grad=True)

    def step():
        s.grad = None
        listwise_loss_from_batch(g, y, s).backward()
    ms = timeit(step)
    print('listwise (fused)  B=%d groups=%d : %.3f ms  %.1f M rows/s' % (B, G, ms, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.1f M rows/s' % (mg, B / mg / 1e3))


def _listmle_torch(g, y, s):
    """The ListMLE loss (all rows take part, no topn, mean over the valid lists) from torch operators: sort by (list, -label), pad to (G, Lmax),
    torch.logcumsumexp, autograd -- what a user writes without rec_block/listmle.py.  One host synchronisation (Lmax) and another for G."""
    B = s.numel()
    _, inv = torch.unique(g, return_inverse=True)
    o = torch.argsort(-y, stable=True)
    o = o[torch.argsort(inv[o], stable=True)]                      # by list, inside a list by label descending, ties by row
    lst, ys, ss = inv[o], y[o], s[o]
    cnt = torch.bincount(lst)
    G, lmax = cnt.numel(), int(cnt.max().item())
    first = torch.cumsum(cnt, 0) - cnt
    col = torch.arange(B, device=s.device) - first[lst]
    pad = torch.full((G, lmax), float('-inf'), device=s.device, dtype=torch.float64)
    pad = pad.index_put((lst, col), ss.double())
    lse = torch.logcumsumexp(pad.flip(1), 1).flip(1)
    per = torch.zeros(G, device=s.device, dtype=torch.float64).index_add(0, lst, lse[lst, col] - ss.double())
    ymax = torch.full((G,), float('-inf'), device=s.device).scatter_reduce(0, lst, ys, 'amax')
    ymin = torch.full((G,), float('inf'), device=s.device).scatter_reduce(0, lst, ys, 'amin')
    valid = (cnt >= 2) & (ymax > ymin)
    return (per * valid).sum() / valid.sum().clamp(min=1)


def listmle():
    """In-batch ListMLE (rec_block/listmle.py) forward + backward beside two yardsticks measured in the same run: the fused softmax
    listwise_loss_from_batch, and the same ListMLE loss from torch operators (_listmle_torch).  Shapes: B = 65 536 in 1024 groups with four label
    levels (the shape of the ranking blocks), and ONE list of 65 536 rows.  Wall time per call and GPU time (the call replayed from a HIP graph;
    the torch composition synchronises the host and cannot be captured); the routes are measured in turn, twice."""
    from rec_now_amd.rec_block.listmle import listmle_loss_from_batch
    from rec_now_amd.rec_block.listwise_loss_from_batch import listwise_loss_from_batch
    rng = np.random.default_rng(6)
    B = 65536
    out = [None]
    for G in (1024, 1):
        g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
        y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
        s = torch.randn(B, device=dev, requires_grad=True)

        def fused():
            s.grad = None
            loss = listmle_loss_from_batch(g, y, s)
            loss.backward()
            out[0] = loss.detach()          # (no reference to the autograd graph stays behind: a capture after an eager step would not end otherwise)

        def softmax():
            s.grad = None
            loss = listwise_loss_from_batch(g, (y > 1.5).float(), s)
            loss.backward()
            out[0] = loss.detach()

        def composed():
            s.grad = None
            loss = _listmle_torch(g, y, s)
            loss.backward()
            out[0] = loss.detach()
        cases = (('listmle fused', fused, True), ('softmax listwise fused', softmax, True), ('listmle torch operators', composed, False))
        res = {name: [] for name, _, _ in cases}
        for run in (1, 2):
            for name, step, capture in cases:
                ms = timeit(step)
                value = float(out[0].item())
                mg = timeit_graph(step) if capture else None
                res[name].append((ms, mg))
                print('run %d  %s B=%d groups=%d value=%.7f : wall %.3f ms per call, GPU %s' % (
                    run, name, B, G, value, ms, ('%.4f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisation: no capture)'))
        f, so, to = (res[name] for name, _, _ in cases)
        print('   groups=%d  wall: torch operators / fused = %.2fx, %.2fx;  fused / softmax = %.2fx, %.2fx;  spread between the two runs, wall: fused %.3f ms, '
              'torch operators %.3f ms' % (G, to[0][0] / f[0][0], to[1][0] / f[1][0], f[0][0] / so[0][0], f[1][0] / so[1][0], abs(f[0][0] - f[1][0]),
                                        abs(to[0][0] - to[1][0])))
        if all(r[1] for r in f + so):
            print('   groups=%d  GPU: fused / softmax = %.2fx, %.2fx;  spread between the two runs, GPU: fused %.4f ms' % (
                G, f[0][1] / so[0][1], f[1][1] / so[1][1], abs(f[0][1] - f[1][1])))


def _approx_ndcg_torch(g, y, s, tau=0.1):
    """The ApproxNDCG loss (all rows take part, exp2 gain, mean over the lists with IDCG > 0) from torch operators: sort by list, pad to
    (G, Lmax), a (G, Lmax, Lmax) sigmoid tensor, autograd -- what a user writes without rec_block/approx_ndcg.py.  float32; one host
    synchronisation (Lmax)."""
    B = s.numel()
    _, inv = torch.unique(g, return_inverse=True)
    o = torch.argsort(inv, stable=True)
    lst, ys, ss = inv[o], y[o], s[o]
    cnt = torch.bincount(lst)
    G, lmax = cnt.numel(), int(cnt.max().item())
    first = torch.cumsum(cnt, 0) - cnt
    col = torch.arange(B, device=s.device) - first[lst]
    real = torch.zeros((G, lmax), dtype=torch.bool, device=s.device).index_put((lst, col), torch.ones((), dtype=torch.bool, device=s.device))
    sp = torch.zeros((G, lmax), device=s.device).index_put((lst, col), ss)
    gain = (torch.exp2(torch.zeros((G, lmax), device=s.device).index_put((lst, col), ys)) - 1.0) * real
    ok = real[:, None, :] & real[:, :, None] & ~torch.eye(lmax, dtype=torch.bool, device=s.device)
    R = (torch.sigmoid((sp[:, None, :] - sp[:, :, None]) / tau) * ok).sum(2)
    adcg = (gain / torch.log2(2.0 + R)).sum(1)
    idcg = (gain.sort(1, descending=True).values / torch.log2(2.0 + torch.arange(lmax, device=s.device))).sum(1)
    valid = idcg > 0
    return -((adcg / idcg.clamp(min=1e-30)) * valid).sum() / valid.sum().clamp(min=1)


def approx_ndcg():
    """In-batch ApproxNDCG (rec_block/approx_ndcg.py) forward + backward beside two yardsticks measured in the same run: the fused BPR loss with
    the NDCG pair weight (pairwise_loss(lambda_weight=NDCGLambdaWeight()): one walk more, the same one exponential per candidate), and the same
    ApproxNDCG loss from torch operators (_approx_ndcg_torch).  Shapes: B = 65 536 in 1024 groups with four label levels, and ONE list of
    65 536 rows (quadratic in the list length on every route; the torch composition would need a 65 536 x 65 536 tensor there and is left
    out).  Wall time per call and GPU time (the call replayed from a HIP graph; the torch composition synchronises the host and cannot be
    captured); the routes are measured in turn, twice."""
    from rec_now_amd.rec_block.approx_ndcg import approx_ndcg_loss
    from rec_now_amd.rec_block.ndcg import NDCGLambdaWeight
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    rng = np.random.default_rng(6)
    B = 65536
    lam = NDCGLambdaWeight()
    out = [None]
    for G in (1024, 1):
        g = torch.from_numpy(rng.integers(0, G, B).astype(np.float32)).to(dev)
        y = torch.from_numpy(rng.integers(0, 4, B).astype(np.float32)).to(dev)
        s = torch.randn(B, device=dev, requires_grad=True)

        def fused():
            s.grad = None
            loss = approx_ndcg_loss(s, y, g)
            loss.backward()
            out[0] = loss.detach()          # (no reference to the autograd graph stays behind: a capture after an eager step would not end otherwise)

        def bpr_lambda():
            s.grad = None
            loss = pairwise_loss(s, y, g, lambda_weight=lam)
            loss.backward()
            out[0] = loss.detach()

        def composed():
            s.grad = None
            loss = _approx_ndcg_torch(g, y, s)
            loss.backward()
            out[0] = loss.detach()
        cases = [('approx_ndcg fused', fused, True), ('BPR + lambda fused', bpr_lambda, True)]
        if G > 1:
            cases.append(('approx_ndcg torch operators', composed, False))
        res = {name: [] for name, _, _ in cases}
        n = reps if G > 1 else max(3, reps // 10)
        for run in (1, 2):
            for name, step, capture in cases:
                ms = timeit(step, n=n, warm=10 if G > 1 else 2)
                value = float(out[0].item())
                mg = timeit_graph(step, n=n) if capture else None
                res[name].append((ms, mg))
                print('run %d  %s B=%d groups=%d value=%.7f : wall %.3f ms per fwd+bwd, GPU %s' % (
                    run, name, B, G, value, ms, ('%.4f ms (graph replay)' % mg) if mg else 'time not separable (host synchronisation: no capture)'))
        f, bl = res['approx_ndcg fused'], res['BPR + lambda fused']
        line = '   groups=%d  wall: approx_ndcg fused / BPR + lambda fused = %.2fx, %.2fx' % (G, f[0][0] / bl[0][0], f[1][0] / bl[1][0])
        if G > 1:
            to = res['approx_ndcg torch operators']
            line += ';  torch operators / fused = %.2fx, %.2fx;  spread between the two runs, wall: fused %.3f ms, torch operators %.3f ms' % (
                to[0][0] / f[0][0], to[1][0] / f[1][0], abs(f[0][0] - f[1][0]), abs(to[0][0] - to[1][0]))
        print(line)
        if all(r[1] for r in f + bl):
            print('   groups=%d  GPU: approx_ndcg fused / BPR + lambda fused = %.2fx, %.2fx;  spread between the two runs, GPU: fused %.4f ms, '
                  'BPR + lambda %.4f ms' % (G, f[0][1] / bl[0][1], f[1][1] / bl[1][1], abs(f[0][1] - f[1][1]), abs(bl[0][1] - bl[1][1])))


def cin():
    from rec_now_amd.layers.cin_layer import CINLayer
    B, F, D, Hs = 16384, 64, 16, [128, 128, 128]          # config 4, one rank's share
    xs = [torch.randn(B, D, device=dev) * 0.1 for _ in range(F)]
    for x in xs:
        x.requires_grad_(True)
    layer = CINLayer(Hs)
    gy = torch.randn(B, D, device=dev)
    layer(xs)

    def step():
        for x in xs:
            x.grad = None
        layer(xs).backward(gy)
    ms = timeit(step, n=max(3, reps // 3))
    ext = [F] + Hs
    fwd = 2.0 * D * F * sum(ext[k - 1] * ext[k] for k in range(1, len(ext))) * B
    n = 3       # round 4: dX_{k-1} and dx0 come out of ONE forward-sized product (csrc/cin_bwd.hip)
    print('CINLayer fwd+bwd  B=%d F=%d D=%d H=%s : %.2f ms  %.1f TFLOP/s executed (%dx fwd flops: 1 fwd + %d bwd products), %.1f TFLOP/s of the 3x-fwd algorithmic flops  %.1f k samples/s'
          % (B, F, D, Hs, ms, n * fwd / ms / 1e9, n, n - 1, 3 * fwd / ms / 1e9, B / ms))


def ple():
    from rec_now_amd.layers.ple_layer import PLELayer
    B, Din = 32768, 4096                                 # config 5, one rank's share (SURVEY-chosen dims)
    x = torch.randn(B, Din, device=dev) * 0.05
    layer = PLELayer(3, [[512, 256], [256, 128]], 2, 1, activation='relu')
    layer(x)

    def step():
        for p in layer.parameters():
            p.grad = None
        outs = layer(x)
        sum(o.sum() for o in outs).backward()
    ms = timeit(step, n=max(3, reps // 3))
    fl = 0.0
    for p in layer.parameters():
        if p.dim() == 3:
            fl += 2.0 * B * p.numel()
        elif p.dim() == 2:
            fl += 2.0 * B * p.numel()
    print('PLELayer fwd+bwd  B=%d Din=%d 3 tasks : %.2f ms  ~%.1f TFLOP/s (3x fwd GEMM flops)  %.1f k samples/s' % (B, Din, ms, 3 * fl / ms / 1e9, B / ms))


def ipnn():
    from rec_now_amd.layers.inner_pnn_layer import InnerPNNLayer
    B, F, D = 131072, 64, 16
    xs = [torch.randn(B, D, device=dev, requires_grad=True) for _ in range(F)]
    P = F * (F - 1) // 2
    gy = torch.randn(B, P, device=dev)
    layer = InnerPNNLayer()

    def step():
        for x in xs:
            x.grad = None
        layer(xs).backward(gy)
    ms = timeit(step)
    print('InnerPNN fwd+bwd  B=%d F=%d D=%d P=%d : %.3f ms  %.0f GB/s algorithmic (8*B*P + 12*B*F*D bytes)  %.1f M samples/s'
          % (B, F, D, P, ms, (8.0 * B * P + 12.0 * B * F * D) / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.0f GB/s' % (mg, (8.0 * B * P + 12.0 * B * F * D) / mg / 1e6))


def senet():
    from rec_now_amd.layers.senet_layer import SENETLayer
    B, F, D = 131072, 64, 16
    xs = [torch.randn(B, D, device=dev, requires_grad=True) for _ in range(F)]
    gy = torch.randn(B, F * D, device=dev)
    layer = SENETLayer(0.25)
    layer(xs)

    def step():
        for x in xs:
            x.grad = None
        layer(xs).backward(gy)
    ms = timeit(step)
    print('SENETLayer fwd+bwd B=%d F=%d D=%d : %.3f ms  %.0f GB/s algorithmic (24*B*F*D bytes: x x2 fwd, x dout x2 + dx bwd)  %.1f M samples/s'
          % (B, F, D, ms, 24.0 * B * F * D / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.0f GB/s' % (mg, 24.0 * B * F * D / mg / 1e6))


def attn():
    from rec_now_amd.rec_block.attention import attention_by_dot_product
    B, L, D = 131072, 50, 16
    u = torch.randn(B, L, D, device=dev, requires_grad=True)
    d = torch.randn(B, D, device=dev, requires_grad=True)
    gm = torch.randn(B, D, device=dev)

    def step():
        u.grad = None
        d.grad = None
        mat, s = attention_by_dot_product(u, d, filter_neg=True)
        (mat * gm).sum().add(s.sum()).backward()
    ms = timeit(step)
    print('attention_by_dot_product fwd+bwd B=%d L=%d D=%d : %.3f ms  %.0f GB/s algorithmic (12*B*L*D bytes)  %.1f M samples/s'
          % (B, L, D, ms, 12.0 * B * L * D / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.0f GB/s' % (mg, 12.0 * B * L * D / mg / 1e6))


def din_ref_eager(u, d, ks, bs):
    """attention_by_dnn as the reference computes it (rec_block/attention.py:62-82): tile + cat, the Dense stack, sigmoid, sums."""
    x = torch.cat([u, d.unsqueeze(1).expand(-1, u.shape[1], -1)], dim=-1)
    for i, (k, b) in enumerate(zip(ks, bs)):
        x = torch.nn.functional.linear(x, k.t(), b)
        if i < len(ks) - 1:
            x = torch.relu(x)
    s = torch.sigmoid(x)
    return (u * s).sum(1), s.squeeze(2).sum(1, keepdim=True)


def din():
    """attention_by_dnn at the attention row's B, L, D with dims [80, 40, 1], and at B 4096, L 100, D 64, dims [200, 80, 1]: forward and
    backward time, TFLOP/s of algorithmic flops (forward 2 B L (D H1 + H1 H2 + H2) + 2 B D H1; backward twice that, the recomputed forward
    not counted) and their fraction of the 157.3 TF exact-fp32 MFMA peak, next to the reference algorithm in torch eager."""
    from rec_now_amd.rec_block.attention import attention_by_dnn
    for B, L, D, dims in ((131072, 50, 16, [80, 40, 1]), (4096, 100, 64, [200, 80, 1])):
        u = (torch.rand(B, L, D, device=dev) - 0.5).requires_grad_(True)
        d = (torch.rand(B, D, device=dev) - 0.5).requires_grad_(True)
        gm, gs = torch.randn(B, D, device=dev), torch.randn(B, 1, device=dev)
        _, _, model = attention_by_dnn(u[:1], d[:1], list(dims))
        ks = [model.named_weights()['layer%d/kernel' % i] for i in range(len(dims))]
        bs = [model.named_weights()['layer%d/bias' % i] for i in range(len(dims))]
        widths = [D] + dims
        flops_f = 2.0 * B * L * sum(widths[i] * widths[i + 1] for i in range(len(dims))) + 2.0 * B * D * dims[0]
        flops_b = 2.0 * flops_f

        def bwd_of(fn):
            mat, ssum = fn()
            loss = (mat * gm).sum() + (ssum * gs).sum()

            def step():
                u.grad = d.grad = None
                model.zero_grad(set_to_none=True)
                loss.backward(retain_graph=True)
            return step

        fused = lambda: model(u, d)                               # noqa: E731
        ref = lambda: din_ref_eager(u, d, ks, bs)                 # noqa: E731
        ms_f, ms_b = timeit(fused), timeit(bwd_of(fused))
        torch.cuda.empty_cache()
        rf, rb = timeit(ref), timeit(bwd_of(ref))
        tf_f, tf_b = flops_f / ms_f / 1e9, flops_b / ms_b / 1e9
        print('attention_by_dnn B=%d L=%d D=%d dims=%s : fwd %.3f ms %.1f TFLOP/s (%.2f of 157.3), bwd %.3f ms %.1f TFLOP/s (%.2f) | '
              'reference in torch eager: fwd %.3f ms, bwd %.3f ms -> speedup fwd %.1fx bwd %.1fx'
              % (B, L, D, dims, ms_f, tf_f, tf_f / 157.3, ms_b, tf_b, tf_b / 157.3, rf, rb, rf / ms_f, rb / ms_b))
        del u, d, model, ks, bs
        torch.cuda.empty_cache()


def focal():
    from rec_now_amd.rec_block.focal_loss import focal_crossentropy_loss
    B = 1 << 22
    x = torch.randn(B, device=dev, requires_grad=True)
    z = (torch.rand(B, device=dev) < 0.25).float()

    def step():
        x.grad = None
        focal_crossentropy_loss(z, x).backward()
    ms = timeit(step)
    print('focal_crossentropy_loss fwd+bwd B=%d : %.3f ms  %.0f GB/s algorithmic (20*B bytes)  %.0f M samples/s' % (B, ms, 20.0 * B / ms / 1e6, B / ms / 1e3))
    mg = timeit_graph(step)
    if mg:
        print('   replayed from a HIP graph (GPU time of the step): %.3f ms  %.0f GB/s' % (mg, 20.0 * B / mg / 1e6))


def embed():
    from rec_now_amd.rec_block.embedding_util import EmbeddingTable, embedding_using_sparse_batch_segment_ids
    B, C, T, D, V = 65536, 100, 64, 16, 1 << 20          # c3: 64 pooled fields x 16-dim from 100 id columns per row
    rng = np.random.default_rng(7)
    slots = torch.from_numpy(rng.integers(0, 80, (B, C)).astype(np.int32)).to(dev)
    ids = torch.from_numpy((rng.zipf(1.3, (B, C)) % V).astype(np.int64)).to(dev)
    table = EmbeddingTable(torch.randn(V, D, device=dev) * 0.05)
    gy = torch.randn(B, T, D, device=dev)
    targets = list(range(T))

    def fwd():
        return embedding_using_sparse_batch_segment_ids(table, slots, targets, ids)

    def step():
        table.weight.grad = None
        fwd().backward(gy)
    ms_f = timeit(fwd)
    ms = timeit(step)
    pooled = float((slots < T).sum().item())
    print('embedding pooled lookup B=%d C=%d T=%d D=%d V=%d : fwd %.3f ms (%.0f GB/s: 4*D bytes gathered per pooled id + 16 B/id + 4*B*T*D out), '
          'fwd+bwd %.3f ms (sort by id + per-id reduction + dense scatter)  %.1f M ids/s'
          % (B, C, T, D, V, ms_f, (pooled * 4 * D + 16.0 * B * C + 4.0 * B * T * D) / ms_f / 1e6, ms, B * C / ms / 1e3))


def star_ref_eager(mode, x, kernel, bias, ps, w):
    """The reference algorithm (star_dense_layer.py:118-163, stacked_dense_layer.py:116-155) in torch eager: a (B, D, U) kernel."""
    B, D = x.shape
    U = kernel.shape[1]
    ks = [p[:, :D * U].view(B, D, U) for p in ps]
    bs = [p[:, D * U:] for p in ps]
    if mode == 'star':
        kf = kernel.unsqueeze(0)
        for k in ks:
            kf = kf * k
        bf = sum(bs) + bias - len(ps)
    else:
        kf = kernel.unsqueeze(0) + w * sum(ks)
        bf = bias + w * sum(bs)
    return torch.bmm(x.unsqueeze(1), kf).squeeze(1) + bf


def star(mode):
    """StarDense / StackedDense at B = 8192, D = 256, U = 128, K = 1 and 2: forward and backward time each, as GB/s of algorithmic bytes
    (forward: K*B*(DU+U)*4 + x + y; backward: the P_k read and the dP_k written, x, dx, y, dy), and the speedup and forward peak-memory
    ratio over the reference algorithm in torch eager."""
    from rec_now_amd.layers.stacked_dense_layer import StackedDenseLayer
    from rec_now_amd.layers.star_dense_layer import StarDenseLayer
    B, D, U = 8192, 256, 128
    R = D * U + U
    for K in (1, 2):
        x = torch.rand(B, D, device=dev, requires_grad=True)
        ps = [(torch.rand(B, R, device=dev) + 0.5).requires_grad_(True) for _ in range(K)]
        gy = torch.randn(B, U, device=dev)
        layer = (StarDenseLayer if mode == 'star' else StackedDenseLayer)(U)
        run = (lambda: layer(x, ps)) if mode == 'star' else (lambda: layer(x, ps, resnet_weight=0.5))
        run()

        def ref():
            return star_ref_eager(mode, x, layer.kernel, layer.bias, ps, 0.5)

        def peak_rise(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            y = fn()
            torch.cuda.synchronize()
            del y
            return torch.cuda.max_memory_allocated() - base

        def bwd_of(fn):
            y = fn()

            def step():
                x.grad = None
                layer.zero_grad(set_to_none=True)
                for p in ps:
                    p.grad = None
                y.backward(gy, retain_graph=True)
            return step

        fwd_bytes = 4.0 * (K * B * R + B * D + B * U)
        bwd_bytes = 4.0 * (2 * K * B * R + 2 * B * D + 2 * B * U)
        ms_f, ms_b = timeit(run), timeit(bwd_of(run))
        rf, rb = timeit(ref), timeit(bwd_of(ref))
        mem, rmem = peak_rise(run), peak_rise(ref)
        print('%s K=%d B=%d D=%d U=%d : fwd %.3f ms %.0f GB/s, bwd %.3f ms %.0f GB/s (algorithmic) | reference in torch eager: fwd %.3f ms, '
              'bwd %.3f ms -> speedup fwd %.1fx bwd %.1fx | forward peak rise %.1f MB vs %.1f MB (%.0fx less)'
              % ('StarDenseLayer' if mode == 'star' else 'StackedDenseLayer', K, B, D, U, ms_f, fwd_bytes / ms_f / 1e6, ms_b,
                 bwd_bytes / ms_b / 1e6, rf, rb, rf / ms_f, rb / ms_b, mem / 2 ** 20, rmem / 2 ** 20, rmem / max(mem, 1)))
        del x, ps, layer
        torch.cuda.empty_cache()


def can_ref_eager(x, params, dims, use_bias=True):
    """The reference algorithm (can_layer.py:243-275) in torch eager with its defaults (tanh between the layers, mask, sum): per layer one
    batched matmul of the (B, L, din) activations against the sample's (B, din, dout) kernel -- the reference's (B, L, 1, din) x (B, 1, din, dout)
    broadcast without an L-fold expanded kernel -- so autograd keeps a (B, L, D_k) activation per layer."""
    B, L, din = x.shape
    h, at = x, 0
    for k, dout in enumerate(dims):
        h = torch.bmm(h, params[:, at:at + din * dout].view(B, din, dout))
        at += din * dout
        if use_bias:
            h = h + params[:, at:at + dout].unsqueeze(1)
            at += dout
        if k + 1 < len(dims):
            h = torch.tanh(h)
        din = dout
    return (h * (x != 0).any(-1, keepdim=True).to(h.dtype)).sum(1)


def can():
    """CANLayer at B = 65 536, L = 50 for D0 16 with [16, 16] and D0 32 with [32, 32, 32] (tanh, bias, mask, sum): forward and forward + backward,
    eager and replayed from a HIP graph, as TB/s of algorithmic bytes (forward: inputs + params + y; backward: those plus g, dx, dparams), beside the
    reference algorithm in torch eager timed in the same run."""
    from rec_now_amd.layers.can_layer import CANLayer
    B, L = 65536, 50
    for D0, dims in ((16, [16, 16]), (32, [32, 32, 32])):
        P, Dn = CANLayer.get_dnn_param_size(D0, dims), dims[-1]
        x = torch.randn(B, L, D0, device=dev)
        x[torch.rand(B, L, device=dev) < 0.2] = 0.0             # padding positions
        x.requires_grad_(True)
        p = (torch.randn(B, P, device=dev) / D0 ** 0.5).requires_grad_(True)
        gy = torch.randn(B, Dn, device=dev)
        layer = CANLayer(dnn_dims=dims)
        run, ref = (lambda: layer(x, p)), (lambda: can_ref_eager(x, p, dims))
        err = (run() - ref()).abs().max().item()

        def fb_of(fn):
            def step():
                x.grad = None
                p.grad = None
                fn().backward(gy)
            return step

        fwd_bytes = 4.0 * (B * L * D0 + B * P + B * Dn)
        fb_bytes = 2 * fwd_bytes + 4.0 * (B * Dn + B * L * D0 + B * P)
        ms_f, ms_fb = timeit(run), timeit(fb_of(run))
        rf, rfb = timeit(ref), timeit(fb_of(ref))
        gf, gfb = timeit_graph(run), timeit_graph(fb_of(run))
        gtxt = 'graph fwd %.3f ms %.2f TB/s, fwd+bwd %.3f ms %.2f TB/s' % (gf, fwd_bytes / gf / 1e9, gfb, fb_bytes / gfb / 1e9) if gf and gfb else 'graph n/a'
        print('CANLayer B=%d L=%d D0=%d dims=%s P=%d : fwd %.3f ms %.2f TB/s, fwd+bwd %.3f ms %.2f TB/s (algorithmic: fwd %.0f MB, fwd+bwd %.0f MB) | %s | '
              'reference in torch eager: fwd %.3f ms, fwd+bwd %.3f ms -> speedup fwd %.1fx, fwd+bwd %.1fx | max |y - eager| %.2g'
              % (B, L, D0, dims, P, ms_f, fwd_bytes / ms_f / 1e9, ms_fb, fb_bytes / ms_fb / 1e9, fwd_bytes / 1e6, fb_bytes / 1e6, gtxt, rf, rfb,
                 rf / ms_f, rfb / ms_fb, err))
        del x, p, layer
        torch.cuda.empty_cache()


def bilinear_ref_eager(xs, W, kind, ii, jj):
    """BilinearInteractionLayer from torch operators: the projection of the left fields in one matmul ('all') or one einsum over the stacked
    weights ('each'), gathered to the pairs -- or, for 'interaction', an einsum over the gathered (B, P, D) left operands -- times the gathered
    right operands."""
    X = torch.stack(xs, 1)                                   # (B, F, D)
    if kind == 'all':
        up = (X[:, :-1] @ W[0])[:, ii]
    elif kind == 'each':
        up = torch.einsum('bfk,fkd->bfd', X[:, :-1], W)[:, ii]
    else:
        up = torch.einsum('bpk,pkd->bpd', X[:, ii], W)
    return (up * X[:, jj]).reshape(X.shape[0], -1)


def bilinear():
    """BilinearInteractionLayer forward + backward (all gradients) at B = 65 536: F 24, D 16 for the three types, then F 40, D 32 for 'all'.  Wall
    time and graph-replay GPU time, the cases in turn, twice, with the spread between the two passes; beside the same layer from torch operators
    in the same run.  GB/s of the byte model: forward 4 B (F D + P D), backward 4 B (2 F D + P D) bytes."""
    from rec_now_amd.layers.bilinear_interaction_layer import BilinearInteractionLayer
    B = 65536
    cases = [(24, 16, 'all'), (24, 16, 'each'), (24, 16, 'interaction'), (40, 32, 'all')]
    seen = {}
    for rnd in (1, 2):
        for F, D, kind in cases:
            P = F * (F - 1) // 2
            xs = [torch.randn(B, D, device=dev, requires_grad=True) for _ in range(F)]
            layer = BilinearInteractionLayer(kind)
            layer([x[:2] for x in xs])
            W = layer.bilinear_weight
            gy = torch.randn(B, P * D, device=dev)
            ii, jj = torch.triu_indices(F, F, 1, device=dev)
            run, ref = (lambda: layer(xs)), (lambda: bilinear_ref_eager(xs, W, kind, ii, jj))
            with torch.no_grad():
                err = (run() - ref()).abs().max().item()

            def fb_of(fn):
                def step():
                    return torch.autograd.grad(fn(), xs + [W], gy)
                return step

            def fwd_of(fn):
                def step():
                    with torch.no_grad():
                        return fn()
                return step
            fwd_bytes, bwd_bytes = 4.0 * B * (F * D + P * D), 4.0 * B * (2 * F * D + P * D)
            fb_bytes = fwd_bytes + bwd_bytes
            ms_f, ms_fb = timeit(fwd_of(run)), timeit(fb_of(run))
            gf, gfb = timeit_graph(fwd_of(run)), timeit_graph(fb_of(run))
            rfb, rgfb = timeit(fb_of(ref)), timeit_graph(fb_of(ref))
            gf, gfb, rgfb = gf or float('nan'), gfb or float('nan'), rgfb or float('nan')
            print('pass %d BilinearInteraction %-11s B=%d F=%d D=%d P=%d : wall fwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | graph fwd %.3f ms %.0f GB/s, '
                  'bwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | torch operators fwd+bwd: wall %.3f ms, graph %.3f ms -> fused is %.2fx (wall) %.2fx (graph) '
                  '| max |y - torch| %.2g' % (rnd, kind, B, F, D, P, ms_f, fwd_bytes / ms_f / 1e6, ms_fb, fb_bytes / ms_fb / 1e6, gf, fwd_bytes / gf / 1e6,
                                            gfb - gf, bwd_bytes / (gfb - gf) / 1e6, gfb, fb_bytes / gfb / 1e6, rfb, rgfb, rfb / ms_fb, rgfb / gfb, err), flush=True)
            seen.setdefault((F, D, kind), []).append((gfb, rgfb))
            del xs, gy, layer, W
            torch.cuda.empty_cache()
    for (F, D, kind), ((a, ra), (b, rb)) in seen.items():
        spread = abs(a - b) / min(a, b)
        worst = min(ra, rb) / max(a, b)
        print('BilinearInteraction %-11s F=%d D=%d : fused fwd+bwd (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; '
              'fused faster in both passes by at least %.1f %% -> %s' % (kind, F, D, a, b, 100 * spread, ra, rb, 100 * (worst - 1),
                                                                       'faster by more than the spread' if worst - 1 > spread else 'NOT faster by more than the spread'))


def autoint_ref_eager(x, Wq, Wk, Wv, Wr, H, d):
    """InteractingLayer from torch operators: three matmuls, the scores and the weighted sum as batched matmuls over the heads, softmax, the
    residual matmul and ReLU."""
    B, F, _ = x.shape
    q, k, v = ((x @ W).reshape(B, F, H, d).transpose(1, 2) for W in (Wq, Wk, Wv))            # (B, H, F, d)
    a = torch.softmax(torch.matmul(q, k.transpose(2, 3)), -1)
    return torch.relu(torch.matmul(a, v).transpose(1, 2).reshape(B, F, H * d) + x @ Wr)


def autoint():
    """InteractingLayer forward + backward (all gradients) at B = 65 536 on a (B, F, D) input: F 24, D 16, H 2, d 8, then F 40, D 32, H 4, d 8.
    Wall time and graph-replay GPU time, the cases in turn, twice, with the spread between the two passes; beside the same layer from torch
    operators (matmul, softmax, autograd) in the same run.  GB/s of the byte model: forward 4 B (F D + F E), backward 4 B (2 F D + F E) bytes."""
    from rec_now_amd.layers.interacting_layer import InteractingLayer
    B = 65536
    cases = [(24, 16, 2, 8), (40, 32, 4, 8)]
    seen = {}
    for rnd in (1, 2):
        for F, D, H, d in cases:
            E = H * d
            x = torch.randn(B, F, D, device=dev, requires_grad=True)
            layer = InteractingLayer(d, H)
            layer(x[:2].detach())
            Ws = [layer.W_query, layer.W_key, layer.W_value, layer.W_res]
            gy = torch.randn(B, F, E, device=dev)
            run, ref = (lambda: layer(x)), (lambda: autoint_ref_eager(x, *Ws, H, d))
            with torch.no_grad():
                err = (run() - ref()).abs().max().item()

            def fb_of(fn):
                def step():
                    return torch.autograd.grad(fn(), [x] + Ws, gy)
                return step

            def fwd_of(fn):
                def step():
                    with torch.no_grad():
                        return fn()
                return step
            fwd_bytes, bwd_bytes = 4.0 * B * (F * D + F * E), 4.0 * B * (2 * F * D + F * E)
            fb_bytes = fwd_bytes + bwd_bytes
            ms_f, ms_fb = timeit(fwd_of(run)), timeit(fb_of(run))
            gf, gfb = timeit_graph(fwd_of(run)), timeit_graph(fb_of(run))
            rf, rfb, rgf, rgfb = timeit(fwd_of(ref)), timeit(fb_of(ref)), timeit_graph(fwd_of(ref)), timeit_graph(fb_of(ref))
            gf, gfb, rgf, rgfb = (v or float('nan') for v in (gf, gfb, rgf, rgfb))
            print('pass %d InteractingLayer B=%d F=%d D=%d H=%d d=%d : wall fwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | graph fwd %.3f ms %.0f GB/s, '
                  'bwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | torch operators: wall fwd %.3f ms, fwd+bwd %.3f ms, graph fwd %.3f ms, fwd+bwd %.3f ms '
                  '-> fused is %.2fx (fwd, graph) %.2fx (fwd+bwd, wall) %.2fx (fwd+bwd, graph) | max |y - torch| %.2g'
                  % (rnd, B, F, D, H, d, ms_f, fwd_bytes / ms_f / 1e6, ms_fb, fb_bytes / ms_fb / 1e6, gf, fwd_bytes / gf / 1e6, gfb - gf,
                     bwd_bytes / (gfb - gf) / 1e6, gfb, fb_bytes / gfb / 1e6, rf, rfb, rgf, rgfb, rgf / gf, rfb / ms_fb, rgfb / gfb, err), flush=True)
            seen.setdefault((F, D, H, d), []).append((gfb, rgfb, gf, rgf))
            del x, gy, layer, Ws
            torch.cuda.empty_cache()
    for (F, D, H, d), ((a, ra, af, raf), (b, rb, bf, rbf)) in seen.items():
        for what, (p, q, rp, rq) in (('fwd', (af, bf, raf, rbf)), ('fwd+bwd', (a, b, ra, rb))):
            spread = abs(p - q) / min(p, q)
            worst = min(rp, rq) / max(p, q)
            print('InteractingLayer F=%d D=%d H=%d d=%d : fused %s (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; '
                  'fused faster in both passes by at least %.1f %% -> %s' % (F, D, H, d, what, p, q, 100 * spread, rp, rq, 100 * (worst - 1),
                                                                           'faster by more than the spread' if worst - 1 > spread else 'NOT faster by more than the spread'))


def afm_ref_eager(x, W, b, h, p, ii, jj):
    """AFMLayer from torch operators: the gathered pair products (B, P, D), the hidden layer as one matmul, ReLU, the scores as a second matmul,
    softmax over the pairs, the weighted sum and the projection."""
    pk = x[:, ii] * x[:, jj]
    a = torch.softmax(torch.relu(pk @ W + b) @ h, 1)        # (B, P, 1)
    return (a * pk).sum(1) @ p


def afm():
    """AFMLayer forward + backward (all gradients) at B = 65 536 on a (B, F, D) input: F 24, D 16, A 16, then F 40, D 32, A 32.  Wall time and
    graph-replay GPU time, the cases in turn, twice, with the spread between the two passes; beside the same layer from torch operators (gather,
    matmul, softmax, autograd) in the same run.  GB/s of the byte model: forward 4 B (F D + D), backward 4 B (2 F D + D) bytes."""
    from rec_now_amd.layers.afm_layer import AFMLayer
    B = 65536
    cases = [(24, 16, 16), (40, 32, 32)]
    seen = {}
    for rnd in (1, 2):
        for F, D, A in cases:
            x = torch.randn(B, F, D, device=dev, requires_grad=True)
            layer = AFMLayer(A)
            layer(x[:2].detach())
            Ws = [layer.attention_W, layer.attention_b, layer.projection_h, layer.projection_p]
            gy = torch.randn(B, 1, device=dev)
            ii, jj = torch.triu_indices(F, F, 1, device=dev)
            run, ref = (lambda: layer(x)), (lambda: afm_ref_eager(x, *Ws, ii, jj))
            with torch.no_grad():
                err = (run() - ref()).abs().max().item()

            def fb_of(fn):
                def step():
                    return torch.autograd.grad(fn(), [x] + Ws, gy)
                return step

            def fwd_of(fn):
                def step():
                    with torch.no_grad():
                        return fn()
                return step
            fwd_bytes, bwd_bytes = 4.0 * B * (F * D + D), 4.0 * B * (2 * F * D + D)
            fb_bytes = fwd_bytes + bwd_bytes
            ms_f, ms_fb = timeit(fwd_of(run)), timeit(fb_of(run))
            gf, gfb = timeit_graph(fwd_of(run)), timeit_graph(fb_of(run))
            rf, rfb, rgf, rgfb = timeit(fwd_of(ref)), timeit(fb_of(ref)), timeit_graph(fwd_of(ref)), timeit_graph(fb_of(ref))
            gf, gfb, rgf, rgfb = (v or float('nan') for v in (gf, gfb, rgf, rgfb))
            print('pass %d AFMLayer B=%d F=%d D=%d A=%d : wall fwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | graph fwd %.3f ms %.0f GB/s, '
                  'bwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | torch operators: wall fwd %.3f ms, fwd+bwd %.3f ms, graph fwd %.3f ms, fwd+bwd %.3f ms '
                  '-> fused is %.2fx (fwd, graph) %.2fx (bwd, graph) %.2fx (fwd+bwd, wall) %.2fx (fwd+bwd, graph) | max |y - torch| %.2g'
                  % (rnd, B, F, D, A, ms_f, fwd_bytes / ms_f / 1e6, ms_fb, fb_bytes / ms_fb / 1e6, gf, fwd_bytes / gf / 1e6, gfb - gf,
                     bwd_bytes / (gfb - gf) / 1e6, gfb, fb_bytes / gfb / 1e6, rf, rfb, rgf, rgfb, rgf / gf, (rgfb - rgf) / (gfb - gf), rfb / ms_fb,
                     rgfb / gfb, err), flush=True)
            seen.setdefault((F, D, A), []).append((gfb, rgfb, gf, rgf))
            del x, gy, layer, Ws
            torch.cuda.empty_cache()
    for (F, D, A), ((a, ra, af, raf), (b, rb, bf, rbf)) in seen.items():
        for what, (p, q, rp, rq) in (('fwd', (af, bf, raf, rbf)), ('bwd', (a - af, b - bf, ra - raf, rb - rbf)), ('fwd+bwd', (a, b, ra, rb))):
            spread = abs(p - q) / min(p, q)
            worst = min(rp, rq) / max(p, q)
            print('AFMLayer F=%d D=%d A=%d : fused %s (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; '
                  'fused faster in both passes by at least %.1f %% -> %s' % (F, D, A, what, p, q, 100 * spread, rp, rq, 100 * (worst - 1),
                                                                           'faster by more than the spread' if worst - 1 > spread else 'NOT faster by more than the spread'))


def ibs_ref_eager(q, v, ids, lq, tau):
    """The in-batch sampled softmax as a user writes it from torch operators: the (B, B) logits, a mask of the accidental hits, cross_entropy."""
    B = q.shape[0]
    logits = q @ v.T / tau
    if lq is not None:
        logits = logits - lq[None, :]
    if ids is not None:
        hit = ids[None, :] == ids[:, None]
        hit.fill_diagonal_(False)
        logits = logits.masked_fill(hit, float('-inf'))
    return torch.nn.functional.cross_entropy(logits, torch.arange(B, device=q.device))


def ibs_graph_ms(fn):
    """GPU time of one step replayed from a captured graph; the graph and what it holds are released before the next measurement."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    ms = timeit(g.replay, reps, warm=2)
    del g
    torch.cuda.empty_cache()
    return ms


def in_batch_softmax():
    """in_batch_softmax_loss forward and forward + backward (dq and dv) at (B 16 384, D 64), (B 65 536, D 64) and (B 65 536, D 128), plain and
    with item ids + log_q: graph-replay GPU time, the routes in turn, twice, with the spread between the two passes; TFLOP/s of the flop model
    (2 B^2 D forward, 8 B^2 D backward) beside the 157.3 TFLOP/s exact-fp32 MFMA peak.  The yardstick is the torch composition in the same run
    (forward, and backward through autograd); at B = 65 536 it holds about 50 GB of (B, B) tensors -- reported as such where it does not fit."""
    from rec_now_amd.rec_block.in_batch_softmax import in_batch_softmax_loss
    tau = 0.5
    cases = [(16384, 64), (65536, 64), (65536, 128)]
    seen = {}
    graph_ms = ibs_graph_ms

    for rnd in (1, 2):
        for B, D in cases:
            for with_ids in (False, True):
                gen = torch.Generator(device=dev).manual_seed(B + D)
                q = (torch.randn(B, D, device=dev, generator=gen) * D ** -0.25).requires_grad_(True)
                v = (torch.randn(B, D, device=dev, generator=gen) * D ** -0.25).requires_grad_(True)
                ids = torch.randint(0, B // 4, (B,), device=dev, generator=gen) if with_ids else None
                lq = torch.rand(B, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids else None
                run, ref = (lambda: in_batch_softmax_loss(q, v, ids, lq, tau)), (lambda: ibs_ref_eager(q, v, ids, lq, tau))

                def fb_of(fn):
                    def step():
                        return torch.autograd.grad(fn(), [q, v])
                    return step

                def fwd_of(fn):
                    def step():
                        with torch.no_grad():
                            return fn()
                    return step
                ff, fb = 2.0 * B * B * D, 8.0 * B * B * D
                gf, gfb = graph_ms(fwd_of(run)), graph_ms(fb_of(run))
                tag = 'ids+log_q' if with_ids else 'plain'
                try:
                    with torch.no_grad():
                        err = abs(run().item() - ref().item())
                    rgf, rgfb = graph_ms(fwd_of(ref)), graph_ms(fb_of(ref))
                    fits = 'torch composition (forms (B, B)): fwd %.3f ms, bwd %.3f ms, fwd+bwd %.3f ms -> fused is %.2fx (fwd) %.2fx (bwd) %.2fx (fwd+bwd) | |loss - torch| %.2g' % (
                        rgf, rgfb - rgf, rgfb, rgf / gf, (rgfb - rgf) / (gfb - gf), rgfb / gfb, err)
                except torch.cuda.OutOfMemoryError:
                    rgf = rgfb = float('nan')
                    fits = 'torch composition: DOES NOT FIT (out of memory on its (B, B) tensors)'
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                print('pass %d in_batch_softmax B=%d D=%d %s : fused (graph) fwd %.3f ms %.1f TFLOP/s (%.2f of 157.3), bwd %.3f ms %.1f TFLOP/s (%.2f), fwd+bwd %.3f ms | %s'
                      % (rnd, B, D, tag, gf, ff / gf / 1e9, ff / gf / 1e9 / 157.3, gfb - gf, fb / (gfb - gf) / 1e9, fb / (gfb - gf) / 1e9 / 157.3, gfb, fits), flush=True)
                seen.setdefault((B, D, tag), []).append((gfb, rgfb, gf, rgf))
                del q, v, ids, lq
                torch.cuda.empty_cache()
    for (B, D, tag), ((a, ra, af, raf), (b, rb, bf, rbf)) in seen.items():
        for what, (p, s, rp, rs) in (('fwd', (af, bf, raf, rbf)), ('bwd', (a - af, b - bf, ra - raf, rb - rbf)), ('fwd+bwd', (a, b, ra, rb))):
            spread = abs(p - s) / min(p, s)
            worst = min(rp, rs) / max(p, s)
            verdict = 'no yardstick' if worst != worst else ('faster by more than the spread' if worst - 1 > spread else 'NOT faster by more than the spread')
            print('in_batch_softmax B=%d D=%d %s : fused %s (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; fused against torch '
                  'in the worse pairing %.2fx -> %s' % (B, D, tag, what, p, s, 100 * spread, rp, rs, worst, verdict))


def ibs_extra_ref_eager(q, v, x, ids, lq, xids, xlq, tau):
    """The in-batch sampled softmax with extra negatives from torch operators: cat, the (B, B + N) logits, a mask of the hits, cross_entropy."""
    B = q.shape[0]
    logits = q @ torch.cat([v, x]).T / tau
    if lq is not None:
        logits = logits - torch.cat([lq, xlq])[None, :]
    if ids is not None:
        hit = torch.cat([ids, xids])[None, :] == ids[:, None]
        hit[:, :B].fill_diagonal_(False)
        logits = logits.masked_fill(hit, float('-inf'))
    return torch.nn.functional.cross_entropy(logits, torch.arange(B, device=q.device))


def in_batch_softmax_extra():
    """in_batch_softmax_loss with extra negatives, forward and forward + backward, at (B 16 384, N 49 152, D 64), (B 65 536, N 65 536, D 64)
    and (B 65 536, N 65 536, D 128); extras trainable (dq, dv and de) and frozen (a memory bank: no de), plain and with ids + log_q.  The
    harness of in_batch_softmax: graph-replay GPU time, the cases in turn, twice, the spread between the passes.  Flop model: forward
    2 B (B + N) D, dq 4 B (B + N) D, dv 4 B^2 D, de 4 B N D, beside the 157.3 TFLOP/s exact-fp32 MFMA peak.  The yardstick is the torch
    composition over the (B, B + N) logits in the same run -- 34 GB a matrix at B = N = 65 536 -- reported as such where it does not fit."""
    from rec_now_amd.rec_block.in_batch_softmax import in_batch_softmax_loss
    tau = 0.5
    cases = [(16384, 49152, 64), (65536, 65536, 64), (65536, 65536, 128)]
    seen = {}
    graph_ms = ibs_graph_ms
    for rnd in (1, 2):
        for B, N, D in cases:
            for frozen in (False, True):
                for with_ids in (False, True):
                    gen = torch.Generator(device=dev).manual_seed(B + D + N)
                    q = (torch.randn(B, D, device=dev, generator=gen) * D ** -0.25).requires_grad_(True)
                    v = (torch.randn(B, D, device=dev, generator=gen) * D ** -0.25).requires_grad_(True)
                    x = (torch.randn(N, D, device=dev, generator=gen) * D ** -0.25).requires_grad_(not frozen)
                    ids = torch.randint(0, B // 4, (B,), device=dev, generator=gen) if with_ids else None
                    xids = torch.randint(0, B // 4, (N,), device=dev, generator=gen) if with_ids else None
                    lq = torch.rand(B, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids else None
                    xlq = torch.rand(N, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids else None
                    run = lambda: in_batch_softmax_loss(q, v, ids, lq, tau, extra_item=x, extra_item_ids=xids, extra_log_q=xlq)      # noqa: E731
                    ref = lambda: ibs_extra_ref_eager(q, v, x, ids, lq, xids, xlq, tau)      # noqa: E731
                    wrt = [q, v] if frozen else [q, v, x]

                    def fb_of(fn):
                        def step():
                            return torch.autograd.grad(fn(), wrt)
                        return step

                    def fwd_of(fn):
                        def step():
                            with torch.no_grad():
                                return fn()
                        return step
                    ff = 2.0 * B * (B + N) * D
                    fb = 4.0 * B * (B + N) * D + 4.0 * B * B * D + (0.0 if frozen else 4.0 * B * N * D)
                    gf, gfb = graph_ms(fwd_of(run)), graph_ms(fb_of(run))
                    tag = ('frozen extras' if frozen else 'trainable extras') + (' ids+log_q' if with_ids else ' plain')
                    try:
                        with torch.no_grad():
                            err = abs(run().item() - ref().item())
                        rgf, rgfb = graph_ms(fwd_of(ref)), graph_ms(fb_of(ref))
                        fits = 'torch composition (forms (B, B + N)): fwd %.3f ms, bwd %.3f ms, fwd+bwd %.3f ms -> fused is %.2fx (fwd) %.2fx (bwd) %.2fx (fwd+bwd) | |loss - torch| %.2g' % (
                            rgf, rgfb - rgf, rgfb, rgf / gf, (rgfb - rgf) / (gfb - gf), rgfb / gfb, err)
                    except torch.cuda.OutOfMemoryError:
                        rgf = rgfb = float('nan')
                        fits = 'torch composition: DID NOT FIT (out of memory on its (B, B + N) tensors)'
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    print('pass %d in_batch_softmax_extra B=%d N=%d D=%d %s : fused (graph) fwd %.3f ms %.1f TFLOP/s (%.2f of 157.3), bwd %.3f ms %.1f TFLOP/s (%.2f), fwd+bwd %.3f ms | %s'
                          % (rnd, B, N, D, tag, gf, ff / gf / 1e9, ff / gf / 1e9 / 157.3, gfb - gf, fb / (gfb - gf) / 1e9, fb / (gfb - gf) / 1e9 / 157.3, gfb, fits), flush=True)
                    seen.setdefault((B, N, D, tag), []).append((gfb, rgfb, gf, rgf))
                    del q, v, x, ids, lq, xids, xlq
                    torch.cuda.empty_cache()
    for (B, N, D, tag), ((a, ra, af, raf), (b, rb, bf, rbf)) in seen.items():
        for what, (p, s, rp, rs) in (('fwd', (af, bf, raf, rbf)), ('bwd', (a - af, b - bf, ra - raf, rb - rbf)), ('fwd+bwd', (a, b, ra, rb))):
            spread = abs(p - s) / min(p, s)
            worst = min(rp, rs) / max(p, s)
            verdict = 'no yardstick' if worst != worst else ('faster by more than the spread' if worst - 1 > spread else 'NOT faster by more than the spread')
            print('in_batch_softmax_extra B=%d N=%d D=%d %s : fused %s (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; fused against '
                  'torch in the worse pairing %.2fx -> %s' % (B, N, D, tag, what, p, s, 100 * spread, rp, rs, worst, verdict))


def ibs_rank_ref_eager(q, v, x, ids, lq, xids, xlq, tau, in_batch):
    """The rank of the positives from torch operators: cat, the (B, B + N) logits, masked_fill of the hits (and of the batch columns where the
    corpus alone holds the candidates), (s > pos).sum(1)."""
    B = q.shape[0]
    s = q @ (v if x is None else torch.cat([v, x])).T / tau
    if lq is not None:
        s = s - (lq if x is None else torch.cat([lq, xlq]))[None, :]
    pos = s.diagonal().clone()
    if ids is not None:
        drop = (ids if x is None else torch.cat([ids, xids]))[None, :] == ids[:, None]
    else:
        drop = torch.zeros(s.shape, dtype=torch.bool, device=s.device)
    if in_batch:
        drop[:, :B].fill_diagonal_(True)
    else:
        drop[:, :B] = True
    return (s.masked_fill(drop, float('-inf')) > pos[:, None]).sum(1)


def in_batch_ranks():
    """in_batch_ranks (the count launch every retrieval metric is made of) at (B 16 384, N 49 152, D 64), (B 65 536, N 65 536, D 64 and 128)
    and the square B 65 536, D 64: plain, with ids + log_q, and once with in_batch_candidates=False (the corpus alone).  The harness of
    in_batch_softmax_extra: graph-replay GPU time, the cases in turn, twice, the spread between the passes.  Two yardsticks in the same run:
    the forward of in_batch_softmax_loss at the same shape (the same tiles and MFMAs plus the exponentials, less the two tiles of the
    positives), and the torch composition over the (B, B + N) logits -- reported as such where it does not fit.  Flop model: 2 B C D with C
    the streamed candidates (B + N, or N for the corpus alone), beside the 157.3 TFLOP/s exact-fp32 MFMA peak."""
    from rec_now_amd.rec_block.in_batch_softmax import in_batch_softmax_loss
    from rec_now_amd.rec_block.retrieval_metrics import in_batch_ranks as ranks
    tau = 0.5
    cases = [(16384, 49152, 64), (65536, 65536, 64), (65536, 65536, 128), (65536, 0, 64)]
    seen = {}
    for rnd in (1, 2):
        for B, N, D in cases:
            for tag, with_ids, in_batch in (('plain', False, True), ('ids+log_q', True, True), ('corpus alone', False, False)):
                if N == 0 and not in_batch:
                    continue
                gen = torch.Generator(device=dev).manual_seed(B + D + N)
                q = torch.randn(B, D, device=dev, generator=gen) * D ** -0.25
                v = torch.randn(B, D, device=dev, generator=gen) * D ** -0.25
                x = torch.randn(N, D, device=dev, generator=gen) * D ** -0.25 if N else None
                ids = torch.randint(0, B // 4, (B,), device=dev, generator=gen) if with_ids else None
                xids = torch.randint(0, B // 4, (N,), device=dev, generator=gen) if with_ids and N else None
                lq = torch.rand(B, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids else None
                xlq = torch.rand(N, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids and N else None
                kw = dict(extra_item=x, extra_item_ids=xids, extra_log_q=xlq)
                run = lambda: ranks(q, v, ids, lq, tau, in_batch_candidates=in_batch, **kw).n_greater      # noqa: E731
                ref = lambda: ibs_rank_ref_eager(q, v, x, ids, lq, xids, xlq, tau, in_batch)      # noqa: E731

                def loss():
                    with torch.no_grad():
                        return in_batch_softmax_loss(q, v, ids, lq, tau, **kw)
                flops = 2.0 * B * ((B if in_batch else 0) + N) * D
                g_rank, g_loss = ibs_graph_ms(run), (ibs_graph_ms(loss) if in_batch else float('nan'))
                try:
                    diff = (run() != ref()).sum().item()
                    g_ref = ibs_graph_ms(ref)
                    fits = 'torch composition (forms (B, B + N)) %.3f ms -> fused is %.2fx | rows whose n_greater differs from torch %d of %d' % (
                        g_ref, g_ref / g_rank, diff, B)
                except torch.cuda.OutOfMemoryError:
                    g_ref = float('nan')
                    fits = 'torch composition: DID NOT FIT (out of memory on its (B, B + N) tensors)'
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                print('pass %d in_batch_ranks B=%d N=%d D=%d %s : ranks (graph) %.3f ms %.1f TFLOP/s (%.2f of 157.3) | loss forward, same shape %.3f ms -> ranks / forward %.3f | %s'
                      % (rnd, B, N, D, tag, g_rank, flops / g_rank / 1e9, flops / g_rank / 1e9 / 157.3, g_loss, g_rank / g_loss, fits), flush=True)
                seen.setdefault((B, N, D, tag), []).append((g_rank, g_loss, g_ref))
                del q, v, x, ids, lq, xids, xlq, kw
                torch.cuda.empty_cache()
    for (B, N, D, tag), ((a, la, ra), (b, lb, rb)) in seen.items():
        spread = max(abs(a - b) / min(a, b), abs(la - lb) / min(la, lb) if la == la else 0.0)
        against = max(a, b) / min(la, lb) if la == la else float('nan')        # the worse pairing: the slower rank pass over the faster forward
        verdict = 'no forward to compare with (the loss has no such candidate set)' if against != against else (
            'no slower than the forward beyond the spread' if against - 1 <= spread else 'SLOWER than the forward beyond the spread')
        print('in_batch_ranks B=%d N=%d D=%d %s : ranks (graph) %.3f / %.3f ms, loss forward %.3f / %.3f ms, largest spread between the passes %.1f %%; '
              'ranks / forward in the worse pairing %.3f -> %s; torch %.3f / %.3f ms, fused against torch in the worse pairing %.2fx'
              % (B, N, D, tag, a, b, la, lb, 100 * spread, against, verdict, ra, rb, min(ra, rb) / max(a, b)))


def ibs_topk_ref_eager(q, v, x, ids, lq, xids, xlq, tau, in_batch, k):
    """The K highest candidates from torch operators: cat, the (B, B + N) logits, masked_fill of the positive and the hits (and of the batch
    columns where the corpus alone holds the candidates), topk."""
    B = q.shape[0]
    s = q @ (v if x is None else torch.cat([v, x])).T / tau
    if lq is not None:
        s = s - (lq if x is None else torch.cat([lq, xlq]))[None, :]
    if ids is not None:
        drop = (ids if x is None else torch.cat([ids, xids]))[None, :] == ids[:, None]
    else:
        drop = torch.zeros(s.shape, dtype=torch.bool, device=s.device)
    if in_batch:
        drop[:, :B].fill_diagonal_(True)
    else:
        drop[:, :B] = True
    return torch.topk(s.masked_fill(drop, float('-inf')), k, dim=1)


def in_batch_top_k():
    """in_batch_top_k at the shapes of in_batch_ranks: plain, with ids + log_q, and the corpus alone, each at K = 10 and K = 100.  The
    harness of in_batch_ranks: graph-replay GPU time, the cases in turn, twice, the spread between the passes.  Two yardsticks in the same
    run: in_batch_ranks at the same shape (the same walk: the ratio is the cost of selection) and the torch composition cat + (B, B + N)
    logits + masked_fill + topk -- reported as such where it does not fit.  Flop model: 2 B C D with C the streamed candidates."""
    from rec_now_amd.rec_block.retrieval_metrics import in_batch_ranks as ranks
    from rec_now_amd.rec_block.retrieval_topk import in_batch_top_k as top_k
    tau = 0.5
    cases = [(16384, 49152, 64), (65536, 65536, 64), (65536, 65536, 128), (65536, 0, 64)]
    seen = {}
    for rnd in (1, 2):
        for B, N, D in cases:
            for tag, with_ids, in_batch in (('plain', False, True), ('ids+log_q', True, True), ('corpus alone', False, False)):
                if N == 0 and not in_batch:
                    continue
                gen = torch.Generator(device=dev).manual_seed(B + D + N)
                q = torch.randn(B, D, device=dev, generator=gen) * D ** -0.25
                v = torch.randn(B, D, device=dev, generator=gen) * D ** -0.25
                x = torch.randn(N, D, device=dev, generator=gen) * D ** -0.25 if N else None
                ids = torch.randint(0, B // 4, (B,), device=dev, generator=gen) if with_ids else None
                xids = torch.randint(0, B // 4, (N,), device=dev, generator=gen) if with_ids and N else None
                lq = torch.rand(B, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids else None
                xlq = torch.rand(N, device=dev, generator=gen).mul_(0.95).add_(0.05).log_() if with_ids and N else None
                kw = dict(extra_item=x, extra_item_ids=xids, extra_log_q=xlq)
                flops = 2.0 * B * ((B if in_batch else 0) + N) * D
                g_rank = ibs_graph_ms(lambda: ranks(q, v, ids, lq, tau, in_batch_candidates=in_batch, **kw).n_greater)
                for k in (10, 100):
                    run = lambda: top_k(q, v, ids, lq, tau, k=k, in_batch_candidates=in_batch, **kw)      # noqa: E731
                    ref = lambda: ibs_topk_ref_eager(q, v, x, ids, lq, xids, xlq, tau, in_batch, k)      # noqa: E731
                    g_top = ibs_graph_ms(run)
                    try:
                        got, (rs, ri) = run(), ref()
                        diff = (got.indices != ri).any(1).sum().item()
                        err = (got.scores - rs).abs().max().item()
                        del got, rs, ri
                        g_ref = ibs_graph_ms(ref)
                        fits = 'torch composition (forms (B, B + N)) %.3f ms -> fused is %.2fx%s | rows whose index list differs from torch %d of %d, max |score - torch| %.2g' % (
                            g_ref, g_ref / g_top, '' if g_ref >= g_top else ' **SLOWER than torch**', diff, B, err)
                    except torch.cuda.OutOfMemoryError:
                        g_ref = float('nan')
                        fits = 'torch composition: DID NOT FIT (out of memory on its (B, B + N) tensors)'
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    print('pass %d in_batch_top_k B=%d N=%d D=%d K=%d %s : top-K (graph) %.3f ms %.1f TFLOP/s (%.2f of 157.3) | in_batch_ranks, same shape %.3f ms -> top-K / ranks %.3f | %s'
                          % (rnd, B, N, D, k, tag, g_top, flops / g_top / 1e9, flops / g_top / 1e9 / 157.3, g_rank, g_top / g_rank, fits), flush=True)
                    seen.setdefault((B, N, D, k, tag), []).append((g_top, g_rank, g_ref))
                del q, v, x, ids, lq, xids, xlq, kw
                torch.cuda.empty_cache()
    for (B, N, D, k, tag), ((a, la, ra), (b, lb, rb)) in seen.items():
        spread = max(abs(a - b) / min(a, b), abs(la - lb) / min(la, lb))
        worst = min(ra, rb) / max(a, b)
        print('in_batch_top_k B=%d N=%d D=%d K=%d %s : top-K (graph) %.3f / %.3f ms, ranks %.3f / %.3f ms, largest spread between the passes %.1f %%; '
              'top-K / ranks %.3f / %.3f; torch %.3f / %.3f ms, fused against torch in the worse pairing %.2fx%s'
              % (B, N, D, k, tag, a, b, la, lb, 100 * spread, a / la, b / lb, ra, rb, worst,
                 '' if worst != worst or worst - 1 > spread else ' -> **NOT faster than torch beyond the spread**'))


def attn_softmax_ref_eager(x, q, lengths, scale):
    """Masked multi-head softmax target attention as a user writes it from torch operators: einsum, masked_fill, softmax, einsum, and the patch
    that zeroes the rows of users with an empty history (their softmax is NaN).  Forms the (B, H, L) scores and keeps the probabilities."""
    s = torch.einsum('bhd,bld->bhl', q, x) * scale
    if lengths is not None:
        key = torch.arange(x.shape[1], device=x.device)[None, :] < lengths[:, None]
        s = s.masked_fill(~key[:, None, :], float('-inf'))
    a = torch.softmax(s, -1)
    if lengths is not None:
        a = torch.where((lengths > 0)[:, None, None], a, torch.zeros_like(a))
    return torch.einsum('bhl,bld->bhd', a, x)


def attention_softmax():
    """attention_by_softmax forward and forward + backward at B 65 536, L 50 / 200, D 16 / 32 / 64, H 1 / 4, without a mask and with lengths
    uniform in 0 .. L: graph-replay GPU time, the cases in turn, twice, with the spread between the two passes.  GB/s under the byte model
    4 B (L D + 2 H D) forward, 4 B (2 L D + 4 H D) backward (with lengths about half of the rows is not read: the model still counts them).
    Yardsticks in the same run: the torch composition (einsum, masked_fill, softmax, einsum, empty-row patch), and for H = 1
    attention_by_dot_product on the same (B, L, D) -- the same stream with less arithmetic, so the ratio is the cost of the softmax."""
    from rec_now_amd.rec_block.attention import attention_by_dot_product, attention_by_softmax
    B = 65536
    seen = {}
    graph_ms = ibs_graph_ms
    for rnd in (1, 2):
        for L in (50, 200):
            for D in (16, 32, 64):
                for H in (1, 4):
                    for with_len in (False, True):
                        gen = torch.Generator(device=dev).manual_seed(L + D + H)
                        x = torch.randn(B, L, D, device=dev, generator=gen).requires_grad_(True)
                        q = torch.randn(B, H, D, device=dev, generator=gen).requires_grad_(True)
                        dc = torch.randn(B, H, D, device=dev, generator=gen)
                        lengths = torch.randint(0, L + 1, (B,), device=dev, generator=gen, dtype=torch.int32) if with_len else None
                        scale = D ** -0.5
                        run, ref = (lambda: attention_by_softmax(x, q, lengths=lengths)), (lambda: attn_softmax_ref_eager(x, q, lengths, scale))

                        def fb_of(fn, leaves=(x, q), g=dc):
                            def step():
                                return torch.autograd.grad(fn(), leaves, g)
                            return step

                        def fwd_of(fn):
                            def step():
                                with torch.no_grad():
                                    return fn()
                            return step
                        bf, bb = 4.0 * B * (L * D + 2 * H * D), 4.0 * B * (2 * L * D + 4 * H * D)
                        gf, gfb = graph_ms(fwd_of(run)), graph_ms(fb_of(run))
                        with torch.no_grad():
                            err = (run() - ref()).abs().max().item()
                        rgf, rgfb = graph_ms(fwd_of(ref)), graph_ms(fb_of(ref))
                        dot = ''
                        df = dfb = float('nan')
                        if H == 1:
                            q2, gm = q.detach()[:, 0].clone().requires_grad_(True), dc[:, 0].contiguous()
                            dot_run = lambda: attention_by_dot_product(x, q2)[0]      # noqa: E731
                            df, dfb = graph_ms(fwd_of(dot_run)), graph_ms(fb_of(dot_run, (x, q2), gm))
                            dot = ' | attention_by_dot_product fwd %.3f ms, fwd+bwd %.3f ms -> softmax / dot %.2fx (fwd) %.2fx (fwd+bwd)' % (df, dfb, gf / df, gfb / dfb)
                            del q2, gm
                        tag = 'lengths' if with_len else 'no mask'
                        print('pass %d attention_softmax L=%d D=%d H=%d %s : fused (graph) fwd %.3f ms %.0f GB/s, bwd %.3f ms %.0f GB/s, fwd+bwd %.3f ms %.0f GB/s | torch '
                              'composition fwd %.3f ms, fwd+bwd %.3f ms -> fused is %.2fx (fwd) %.2fx (fwd+bwd) | max |out - torch| %.2g%s'
                              % (rnd, L, D, H, tag, gf, bf / gf / 1e6, gfb - gf, bb / (gfb - gf) / 1e6, gfb, (bf + bb) / gfb / 1e6, rgf, rgfb, rgf / gf, rgfb / gfb, err, dot),
                              flush=True)
                        seen.setdefault((L, D, H, tag), []).append((gf, gfb, rgf, rgfb, df, dfb))
                        del x, q, dc, lengths
                        torch.cuda.empty_cache()
    for (L, D, H, tag), (a, b) in seen.items():
        for what, i in (('fwd', 0), ('fwd+bwd', 1)):
            p, s_, rp, rs = a[i], b[i], a[i + 2], b[i + 2]
            spread = abs(p - s_) / min(p, s_)
            worst = min(rp, rs) / max(p, s_)
            verdict = 'faster by more than the spread' if worst - 1 > spread else '**NOT faster than torch by more than the spread**'
            line = ('attention_softmax L=%d D=%d H=%d %s : fused %s (graph) %.3f / %.3f ms, spread between the passes %.1f %%; torch %.3f / %.3f ms; fused against '
                    'torch in the worse pairing %.2fx -> %s' % (L, D, H, tag, what, p, s_, 100 * spread, rp, rs, worst, verdict))
            if H == 1:
                line += '; against attention_by_dot_product %.2fx / %.2fx of its time' % (p / a[i + 4], s_ / b[i + 4])
            print(line)


def gnn_ref_eager(x, indices, ws, L, F):
    """The reference algorithm (sparse_gnn_layer.py:183-236) in torch eager: transpose to (B, D, F), per layer a dense (F, F) matrix scattered
    from the weight vector, matmul, add, tanh; transpose back and flatten."""
    o = x.transpose(1, 2).contiguous()                      # tf.transpose is a physical transpose
    for i in range(L):
        W = torch.zeros(F, F, device=x.device).index_put((indices[:, 0], indices[:, 1]), ws[i % len(ws)])
        o = torch.tanh(o + torch.matmul(o, W))
    return o.transpose(1, 2).reshape(x.shape[0], -1)


def gnn():
    """SparseGNNLayer at B = 65536, D = 32, L = 3, tanh, unshared weights, on circulant graphs (node i aggregates its k nearest neighbours; k = 2 is
    the ring, k = F - 1 the complete graph): F 32 with in-degree 2, 4, 8, 16, 31, F 64 with 8, 32, 63, F 128 complete.  Per graph the edge route
    (csrc/sparse_gnn.hip, F <= 64), the dense MFMA route (csrc/sparse_gnn_dense.hip) and the reference algorithm in torch eager, timed in the
    same run in both orders (edges, dense, reference, reference, dense, edges; the two figures of each are averaged): forward and backward
    time each, TB/s of algorithmic bytes (forward 2 B F D 4: x read, y written; backward 3 B F D 4: x and dy read, dx written) and for the
    dense route TFLOP/s of its MFMA work (forward 2 B D F^2 L; backward three times that: the recomputed chain, dz M^T and dM).  First line:
    the plain-stream rate of the same run (a device copy of the F 32 input)."""
    import logging
    from rec_now_amd.layers.sparse_gnn_layer import SparseGNNLayer
    B, D, L = 65536, 32, 3
    logging.getLogger().setLevel(logging.ERROR)       # F == D = 32: the layer warns on every call that it reads the input as (B, F, D)
    src = torch.randn(B, 32 * D, device=dev)
    ms = timeit(lambda: src.clone())
    print('plain stream (clone of %d MB): %.3f ms, %.2f TB/s read + written' % (src.numel() * 4 >> 20, ms, 2 * 4.0 * src.numel() / ms / 1e9))
    del src
    for F, k in ((32, 2), (32, 4), (32, 8), (32, 16), (32, 31), (64, 8), (64, 32), (64, 63), (128, 127)):
        offs = [o for j in range(1, k // 2 + 1) for o in (-j, j)] + ([k // 2 + 1] if k % 2 else [])
        nbrs = {i: sorted((i + o) % F for o in offs) for i in range(F)}
        x = (torch.randn(B, F, D, device=dev) * 0.5).requires_grad_(True)
        gy = torch.randn(B, F * D, device=dev)
        layers = {r: SparseGNNLayer(list(range(F)), nbrs, num_layers=L, share_weights_between_layers=False, activation='tanh', route=r)
                  for r in (('edges', 'dense') if F <= 64 else ('dense',))}
        dense = layers['dense']
        dense(x[:8])
        E = len(dense.indices)
        assert E == k * F
        with torch.no_grad():
            for v in dense.named_weights().values():
                v.mul_(min(1.0, 8.0 / k))
        for lay in layers.values():
            lay(x[:8])
            lay.load_state_dict(dense.state_dict())
        ix = torch.tensor(dense.indices, device=dev)
        fns = {r: (lambda lay=lay: lay(x)) for r, lay in layers.items()}
        fns['ref'] = lambda: gnn_ref_eager(x, ix, dense.gnn_weights, L, F)
        err = {r: float((fns[r]() - fns['ref']()).detach().abs().max()) for r in layers}

        def bwd_of(fn):
            y = fn()

            def step():
                x.grad = None
                for lay in layers.values():
                    lay.zero_grad(set_to_none=True)
                y.backward(gy, retain_graph=True)
            return step

        order = [r for r in ('edges', 'dense', 'ref') if r in fns]
        t = {r: [] for r in order}
        for r in order + order[::-1]:
            t[r].append((timeit(fns[r]), timeit(bwd_of(fns[r]))))
        nbytes, flops = 4.0 * B * F * D, 2.0 * B * D * F * F * L
        rf, rb = (t['ref'][0][0] + t['ref'][1][0]) / 2, (t['ref'][0][1] + t['ref'][1][1]) / 2
        print('SparseGNNLayer F=%d in-degree %d E=%d B=%d D=%d L=%d tanh unshared | reference in torch eager: fwd %.3f ms, bwd %.3f ms'
              % (F, k, E, B, D, L, rf, rb))
        for r in layers:
            (f1, b1), (f2, b2) = t[r]
            ms_f, ms_b = (f1 + f2) / 2, (b1 + b2) / 2
            mfma = ', MFMA fwd %.1f bwd %.1f TFLOP/s' % (flops / ms_f / 1e9, 3 * flops / ms_b / 1e9) if r == 'dense' else ''
            print('    %-5s: fwd %.3f ms %.2f TB/s, bwd %.3f ms %.2f TB/s (algorithmic)%s | against eager fwd %.1fx bwd %.1fx fwd+bwd %.1fx | '
                  'runs fwd %.3f / %.3f, bwd %.3f / %.3f ms | max |y - eager| %.2g'
                  % (r, ms_f, 2 * nbytes / ms_f / 1e9, ms_b, 3 * nbytes / ms_b / 1e9, mfma, rf / ms_f, rb / ms_b, (rf + rb) / (ms_f + ms_b),
                     f1, f2, b1, b2, err[r]))
        del x, gy, layers, dense, fns
        torch.cuda.empty_cache()


def hash():
    """FastMultiHashLayer at B = 65536, L = 50, num_hash = 2, num_bins = 2^20, D = 8 and 32: `get` ((B, L, D)) and `get_pooling` ((B, D), weighted),
    forward and forward + backward (d table, and d weights for the pooling).  Byte model: ids once (8 B each), num_hash table rows per id of 4 D
    bytes rounded up to the 64 B a row fetch costs at least, the output once.  Baseline: the lookup half of the reference algorithm in torch eager
    on PRECOMPUTED buckets -- table[buckets].sum(-2) (times weights, .sum(1)) -- which is handed what the reference hashes on the host and skips its
    host-to-device copy."""
    from rec_now_amd.layers.multi_hash_layer import FastMultiHashLayer
    B, L, nh, nb = 65536, 50, 2, 1 << 20
    for D in (8, 32):
        ids = torch.randint(0, 1 << 40, (B, L), device=dev)
        w = torch.randn(B, L, device=dev, requires_grad=True)
        layer = FastMultiHashLayer(nb, D, num_hash=nh, embeddings_initializer='random_normal')
        layer.get(ids[:4])
        table = layer.tables[0]
        plain = FastMultiHashLayer(nb, -1, num_hash=nh)
        buckets = plain(ids, combiner=None).reshape(B, nh, L).permute(0, 2, 1).contiguous() + torch.arange(nh, device=dev) * nb      # (B, L, nh) rows
        g_get, g_pool = torch.randn(B, L, D, device=dev), torch.randn(B, D, device=dev)
        row = max(4 * D, 64)
        cases = (('get', lambda: layer.get(ids), lambda: table[buckets].sum(-2), g_get, 8.0 * B * L + nh * row * B * L + 4.0 * B * L * D),
                 ('get_pooling', lambda: layer.get_pooling(ids, w), lambda: (w[..., None] * table[buckets].sum(-2)).sum(1), g_pool,
                  12.0 * B * L + nh * row * B * L + 4.0 * B * D))
        for name, run, ref, gy, nbytes in cases:
            def fb_of(fn):
                def step():
                    table.grad = None
                    w.grad = None
                    fn().backward(gy)
                return step
            # both orders: fused, reference, reference, fused; the two figures of each are averaged
            f1, b1 = timeit(run), timeit(fb_of(run))
            r1, rb1 = timeit(ref), timeit(fb_of(ref))
            r2, rb2 = timeit(ref), timeit(fb_of(ref))
            f2, b2 = timeit(run), timeit(fb_of(run))
            ms_f, ms_b, rf, rb = (f1 + f2) / 2, (b1 + b2) / 2, (r1 + r2) / 2, (rb1 + rb2) / 2
            print('FastMultiHashLayer.%-11s B=%d L=%d D=%d num_hash=%d num_bins=2^20 : fwd %.3f ms %.2f TB/s (byte model %.0f MB), fwd+bwd %.3f ms | torch eager on '
                  'precomputed buckets: fwd %.3f ms, fwd+bwd %.3f ms -> ratio fwd %.2fx fwd+bwd %.2fx | runs fwd %.3f / %.3f, fwd+bwd %.3f / %.3f ms'
                  % (name, B, L, D, nh, ms_f, nbytes / ms_f / 1e9, nbytes / 1e6, ms_b, rf, rb, rf / ms_f, rb / ms_b, f1, f2, b1, b2))
        hs = timeit(lambda: plain(ids, combiner=None))
        print('FastMultiHashLayer bucket numbers only (embedding_dim -1) B=%d L=%d num_hash=%d : %.3f ms, %.2f G ids/s' % (B, L, nh, hs, B * L / hs / 1e6))
        del ids, w, layer, table, buckets, g_get, g_pool
        torch.cuda.empty_cache()


def cross():
    """CartesianProductLayer -> MultiHashLayer at B = 65536, two int64 inputs of 10 and 5 ids (P = 50 crossed ids per row, the L of the `hash` row),
    num_hash = 2, num_bins = 2^20, D = 8 and 32: `call(sum)` ((B, P, D)) and `get_pooling` ((B, D), weighted), forward and forward + backward.  Beside
    it, in the same run: (a) the same layer on a precomputed (B, 50) int64 id tensor -- the plain-id kernel, so the difference is what composing and
    hashing the two to three times longer text costs (the crossed launch reads 15 ids per row instead of 50); (b) the host route: the (B, P) Python
    strings, hash_strings_host, the upload of the (B, P, num_hash) buckets and the gather, timed once each (seconds, not milliseconds)."""
    import time
    from rec_now_amd.layers import CartesianProductLayer, MultiHashLayer
    from rec_now_amd.layers.multi_hash_layer import MODE_SUM, _BUCKETS, hash_strings_host
    B, L1, L2, nh, nb = 65536, 10, 5, 2, 1 << 20
    P = L1 * L2
    a, b = torch.randint(0, 1 << 40, (B, L1), device=dev), torch.randint(0, 1 << 40, (B, L2), device=dev)
    ids = torch.randint(0, 1 << 40, (B, P), device=dev)
    product = CartesianProductLayer()
    crossed = product([a, b])
    t0 = time.perf_counter()
    strs = product([a.cpu().numpy(), b.cpu().numpy()])
    t1 = time.perf_counter()
    bk = hash_strings_host(strs.reshape(-1).tolist(), nb, [1, 2], False)
    t2 = time.perf_counter()
    print('host route B=%d P=%d: Python strings %.2f s, hash_strings_host %.2f s (mean text %.1f bytes)'
          % (B, P, t1 - t0, t2 - t1, sum(len(t) for t in strs[:64].reshape(-1)) / (64.0 * P)))
    for D in (8, 32):
        w = torch.randn(B, P, device=dev, requires_grad=True)
        layer = MultiHashLayer(nb, D, num_hash=nh, embeddings_initializer='random_normal')
        layer.get(ids[:4])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        layer._embed(bk, _BUCKETS, (B, P), MODE_SUM)
        torch.cuda.synchronize()
        print('host route D=%d: bucket upload + gather %.1f ms' % (D, (time.perf_counter() - t3) * 1e3))
        g_sum, g_pool = torch.randn(B, P, D, device=dev), torch.randn(B, D, device=dev)
        cases = (('call(sum)', lambda: layer(crossed, combiner='sum'), lambda: layer(ids, combiner='sum'), g_sum),
                 ('get_pooling', lambda: layer.get_pooling(crossed, w), lambda: layer.get_pooling(ids, w), g_pool))
        for name, run, ref, gy in cases:
            def fb_of(fn):
                def step():
                    for t in layer.tables:
                        t.grad = None
                    w.grad = None
                    fn().backward(gy)
                return step
            # both orders: crossed, plain ids, plain ids, crossed; the two figures of each are averaged
            f1, b1 = timeit(run), timeit(fb_of(run))
            r1, rb1 = timeit(ref), timeit(fb_of(ref))
            r2, rb2 = timeit(ref), timeit(fb_of(ref))
            f2, b2 = timeit(run), timeit(fb_of(run))
            ms_f, ms_b, rf, rb = (f1 + f2) / 2, (b1 + b2) / 2, (r1 + r2) / 2, (rb1 + rb2) / 2
            print('MultiHashLayer.%-11s on CrossedIds B=%d (10 x 5 int64) D=%d num_hash=%d num_bins=2^20 : fwd %.3f ms, fwd+bwd %.3f ms | the same on a (B, 50) id '
                  'tensor: fwd %.3f ms, fwd+bwd %.3f ms -> crossed / plain fwd %.2fx fwd+bwd %.2fx | runs crossed fwd %.3f / %.3f, fwd+bwd %.3f / %.3f, plain fwd '
                  '%.3f / %.3f, fwd+bwd %.3f / %.3f ms' % (name, B, D, nh, ms_f, ms_b, rf, rb, ms_f / rf, ms_b / rb, f1, f2, b1, b2, r1, r2, rb1, rb2))
        del w, layer, g_sum, g_pool
        torch.cuda.empty_cache()
    plain = MultiHashLayer(nb, -1, num_hash=nh)
    hs, hp = timeit(lambda: plain(crossed, combiner='concat')), timeit(lambda: plain(ids, combiner='concat'))
    tx = timeit(lambda: crossed.text_bytes())
    print('MultiHashLayer bucket numbers only B=%d P=%d num_hash=%d : crossed %.3f ms, plain ids %.3f ms; CrossedIds.text_bytes() %.3f ms' % (B, P, nh, hs, hp, tx))


def slot():
    """fetch_single_slot, embedding_single_slot (forward, forward + backward) and pool_slots (T = 24) at B = 65536, C = 128, ncols = 50, V = 2^20,
    D = 8 and 32; the target slot occurs 0..40 times per row (mean about 20).  Byte model (algorithmic): the (B, C) inputs read once, the outputs
    written once, each selected table row gathered once.  Baseline: the reference route restated in torch eager on the same GPU -- boolean_mask,
    unique, gather, pad by scatter (segment reductions by scatter_reduce / index_add for pool_slots)."""
    from rec_now_amd.rec_block.embedding_util import EmbeddingTable, embedding_single_slot, fetch_single_slot, pool_slots
    B, C, ncols, V, T, target = 65536, 128, 50, 1 << 20, 24, 7
    rng = np.random.default_rng(0)
    count = rng.integers(0, 41, B)
    place = np.argsort(rng.random((B, C)), axis=1)                                     # rank of a column: the slot sits in `count` random columns
    other = rng.integers(100, 100 + 3 * T, (B, C))
    slots_np = np.where(place < count[:, None], target, other).astype(np.int32)
    slots = torch.from_numpy(slots_np).to(dev)
    ids = torch.randint(0, V, (B, C), device=dev)
    w = torch.randn(B, C, device=dev, requires_grad=True)
    n_sel = int(np.minimum(count, ncols).sum())
    pool_targets = list(range(100, 100 + T))
    col = torch.arange(ncols, device=dev)

    def ragged(mask):
        rows = mask.nonzero()[:, 0]
        first = torch.cumsum(mask.sum(1), 0) - mask.sum(1)
        pos = torch.arange(rows.numel(), device=dev) - first[rows]
        return rows, pos, pos < ncols

    def eager_fetch():
        mask = slots == target
        rows, pos, keep = ragged(mask)
        oi = torch.zeros(B, ncols, dtype=ids.dtype, device=dev)
        ow = torch.zeros(B, ncols, device=dev)
        oi[rows[keep], pos[keep]] = ids[mask][keep]
        ow = ow.index_put((rows[keep], pos[keep]), w[mask][keep])
        return oi, ow

    def eager_embed(weight):
        mask = slots == target
        rows, pos, keep = ragged(mask)
        uniq, inv = torch.unique(ids[mask], return_inverse=True)
        emb = weight[uniq][inv]
        out = torch.zeros(B, ncols, weight.shape[1], device=dev).index_put((rows[keep], pos[keep]), emb[keep])
        ow = torch.zeros(B, ncols, device=dev).index_put((rows[keep], pos[keep]), w[mask][keep])
        om = torch.zeros(B, ncols, dtype=torch.bool, device=dev)
        om[rows[keep], pos[keep]] = True
        return out, ow.unsqueeze(-1), om.unsqueeze(-1)

    tg = torch.tensor(pool_targets, device=dev, dtype=torch.int32)

    def eager_pool():
        hit = slots.unsqueeze(-1) == tg
        seg = torch.where(hit.any(-1), hit.int().argmax(-1) + torch.arange(B, device=dev).unsqueeze(1) * T, -1)
        keep = seg >= 0
        s = seg[keep]
        pi = torch.full((B * T,), torch.iinfo(ids.dtype).max, dtype=ids.dtype, device=dev).scatter_reduce(0, s, ids[keep], 'amin')
        pi = torch.where(pi != torch.iinfo(ids.dtype).max, pi, 0)
        pw = torch.zeros(B * T, device=dev).index_add(0, s, w[keep])
        return pi.reshape(B, T), pw.reshape(B, T)

    def both(run, ref):
        f1 = timeit(run)
        r1 = timeit(ref)
        r2 = timeit(ref)
        f2 = timeit(run)
        return (f1 + f2) / 2, (r1 + r2) / 2

    with torch.no_grad():
        ms, ref = both(lambda: fetch_single_slot(slots, target, ids, w, ncols=ncols), eager_fetch)
    nbytes = 4.0 * B * C + 12.0 * n_sel + 12.0 * B * ncols                           # slots; selected ids + weights; ids + weights out
    print('slot fetch_single_slot     B=%d C=%d ncols=%d : %.3f ms %.2f TB/s (byte model %.0f MB) | torch eager %.3f ms -> %.2fx'
          % (B, C, ncols, ms, nbytes / ms / 1e9, nbytes / 1e6, ref, ref / ms))
    with torch.no_grad():
        ms, ref = both(lambda: pool_slots(slots, pool_targets, ids, w), eager_pool)
    n_pool = float(np.isin(slots_np, pool_targets).sum())
    nbytes = 4.0 * B * C + 12.0 * n_pool + 12.0 * B * T
    print('slot pool_slots T=%d       B=%d C=%d : %.3f ms %.2f TB/s (byte model %.0f MB) | torch eager %.3f ms -> %.2fx'
          % (T, B, C, ms, nbytes / ms / 1e9, nbytes / 1e6, ref, ref / ms))
    for D in (8, 32):
        table = EmbeddingTable(torch.randn(V, D, device=dev) * 0.05)
        ge, gw = torch.randn(B, ncols, D, device=dev), torch.randn(B, ncols, 1, device=dev)
        run = lambda: embedding_single_slot(table, slots, target, ids, w, ncols=ncols)             # noqa: E731
        refrun = lambda: eager_embed(table.weight)                                                 # noqa: E731

        def fb_of(fn):
            def step():
                table.weight.grad = None
                w.grad = None
                e, wt, _ = fn()
                torch.autograd.backward([e, wt], [ge, gw])
            return step
        with torch.no_grad():
            ms_f, ref_f = both(run, refrun)
        ms_b, ref_b = both(fb_of(run), fb_of(refrun))
        nbytes = 4.0 * B * C + n_sel * (12.0 + 4.0 * D) + B * ncols * (4.0 * D + 5.0)     # slots; selected id, weight, table row; out, weights, mask
        print('slot embedding_single_slot B=%d C=%d ncols=%d D=%d V=2^20 : fwd %.3f ms %.2f TB/s (byte model %.0f MB), fwd+bwd %.3f ms | torch eager fwd %.3f ms, '
              'fwd+bwd %.3f ms -> ratio fwd %.2fx fwd+bwd %.2fx' % (B, C, ncols, D, ms_f, nbytes / ms_f / 1e9, nbytes / 1e6, ms_b, ref_f, ref_b, ref_f / ms_f, ref_b / ms_b))
        del table, ge, gw
        torch.cuda.empty_cache()


def tensor_util():
    """PoolingLayer, pad_or_truncate and the element-wise embedding weights at B = 65536: forward and forward + backward, eager and replayed from a
    graph, each beside the same op written with torch's own operators (sum / mean / amax / amin, F.pad / slicing, w[:, pos]) timed in the same run.
    Byte model (algorithmic): every input read once, every output written once; the backward adds the output gradient read and the input gradient(s)
    written (max / min read x and y again).  Set the TB/s beside the plain-stream rate of tools/micro/stream_bench.py on the same box."""
    import torch.nn.functional as F
    from rec_now_amd.layers import PoolingLayer
    from rec_now_amd.layers.fix_length_layer import pad_or_truncate
    from rec_now_amd.rec_block.embedding_wise_weight import apply_embedding_element_wise_weight, gather_embedding_element_wise_weight
    B = 65536

    def row(tag, run, ref, args, grads, bytes_f, bytes_b):
        """run / ref: functions of the differentiable inputs `args`; grads: they carry a gradient (False: forward only)."""
        def fwd(fn):
            def step():
                with torch.no_grad():
                    return fn(*args)
            return step

        def fb(fn):
            def step():
                for a in args:
                    a.grad = None
                y = fn(*args)
                y.backward(g)
            return step
        g = torch.randn_like(run(*args)) if grads else None
        cols = []
        for make, nbytes in ((fwd, bytes_f),) + (((fb, bytes_f + bytes_b),) if grads else ()):
            e1, r1 = timeit(make(run)), timeit(make(ref))
            r2, e2 = timeit(make(ref)), timeit(make(run))
            ge, gr = timeit_graph(make(run)), timeit_graph(make(ref))
            cols.append((nbytes, (e1 + e2) / 2, (r1 + r2) / 2, ge, gr))
        for name, (nbytes, e, r, ge, gr) in zip(('fwd    ', 'fwd+bwd'), cols):
            gtxt = 'graph %.3f ms %.2f TB/s | torch graph %.3f ms -> %.2fx' % (ge, nbytes / ge / 1e9, gr, gr / ge) if ge and gr else 'graph n/a'
            print('tensor_util %-34s %s : eager %.3f ms | torch eager %.3f ms -> %.2fx | %s (byte model %.0f MB)'
                  % (tag, name, e, r, r / e, gtxt, nbytes / 1e6))

    x = torch.randn(B, 50, 32, device=dev, requires_grad=True)
    nin, nout = 4.0 * x.numel(), 4.0 * B * 32
    torch_ops = {'sum': lambda t: t.sum(1), 'mean': lambda t: t.mean(1), 'max': lambda t: t.amax(1), 'min': lambda t: t.amin(1)}
    for combiner in ('sum', 'mean', 'max', 'min'):
        layer = PoolingLayer(axis=1, combiner=combiner)
        extra = nin + nout if combiner in ('max', 'min') else 0.0
        row('PoolingLayer %s (B,50,32) axis 1' % combiner, layer, torch_ops[combiner], (x,), True, nin + nout, nout + nin + extra)
    del x
    x = torch.randn(B, 37, 32, device=dev, requires_grad=True)
    row('pad_or_truncate (B,37,32) -> 50', lambda t: pad_or_truncate(t, 50, axis=1), lambda t: F.pad(t, (0, 0, 0, 13)), (x,), True,
        4.0 * B * 32 * (37 + 50), 4.0 * B * 32 * (37 + 50))
    ids = torch.randint(0, 1 << 40, (B, 80), device=dev)
    row('pad_or_truncate (B,80) int64 -> 50', lambda t: pad_or_truncate(t, 50), lambda t: t[:, :50].contiguous(), (ids,), False, 8.0 * B * 100, 0.0)
    del x, ids
    E, P = 64, 1024
    pos = np.repeat(np.arange(E), P // E).tolist()
    pos_t = torch.tensor(pos, device=dev)
    w = torch.randn(B, E, device=dev, requires_grad=True)
    xin = torch.randn(B, P, device=dev, requires_grad=True)
    row('gather element-wise weight E=64 P=1024', lambda t: gather_embedding_element_wise_weight(t, pos), lambda t: t[:, pos_t], (w,), True,
        4.0 * B * (E + P), 4.0 * B * (E + P))
    row('apply element-wise weight E=64 P=1024', lambda a, t: apply_embedding_element_wise_weight(a, t, pos), lambda a, t: a * t[:, pos_t], (xin, w), True,
        4.0 * B * (E + 2 * P), 4.0 * B * (3 * P + 2 * E + P))


if __name__ == '__main__':
    which = sys.argv[2].split(',') if len(sys.argv) > 2 else ['fm', 'dcn', 'pair', 'list', 'cin', 'ple', 'star', 'stacked', 'gnn', 'ipnn', 'senet', 'attn', 'din', 'focal', 'embed']
    if 'fm' in which:
        fm()
    if 'dcn' in which:
        dcn()
    if 'pair' in which:
        pairwise(8192, 128, 'config2')
        pairwise(8192, 0, 'config2-skewed (Zipf 1.2 group sizes, cap 2048)')
        pairwise(65536, 1024, 'config3')
        pairwise(65536, 0, 'config3-skewed (Zipf 1.2 group sizes, cap 2048)')
    if 'pair_table' in which:
        pair_table()
    if 'pair_kind' in which:
        pair_kind()
    if 'pair_lambda' in which:
        pair_lambda()
    if 'pair_auc' in which:
        pair_auc()
    if 'pair_auc_sort' in which:
        pair_auc_sort()
    if 'list' in which:
        listwise()
    if 'listmle' in which:
        listmle()
    if 'approx_ndcg' in which:
        approx_ndcg()
    if 'cin' in which:
        cin()
    if 'ple' in which:
        ple()
    for mode in ('star', 'stacked'):
        if mode in which:
            star(mode)
    if 'gnn' in which:
        gnn()
    for name, fn in (('ipnn', ipnn), ('senet', senet), ('attn', attn), ('din', din), ('focal', focal), ('embed', embed), ('hash', hash), ('cross', cross), ('slot', slot), ('tensor_util', tensor_util), ('can', can), ('bilinear', bilinear), ('autoint', autoint), ('afm', afm), ('in_batch_softmax', in_batch_softmax), ('in_batch_softmax_extra', in_batch_softmax_extra), ('in_batch_ranks', in_batch_ranks), ('in_batch_top_k', in_batch_top_k), ('attention_softmax', attention_softmax)):
        if name in which:
            fn()

"""GPU parity of the whole-step entry `recnow_dcn_mix_step` (rec_now_amd/step.py): x -> DCNMixLayer ->
MultiDenseLayer(1,1) -> pairwise_loss and every gradient, enqueued phase by phase from C on buffers allocated once.

  * against the drop-in autograd route (same kernels: loss, scores and every gradient but the head bias bit for bit);
  * at the PER-RANK shard sizes of the metric's 4- and 8-GPU rows (16 384 and 8192 rows x 1024: the dispatcher splits K of the
    M = B products there) against the fp64 chunked oracle + the C pair oracle, through the data-parallel form: a 1-rank RCCL
    group with the collectives forced on, gradients written into the LayerwiseReducer's buckets, statistics in the first
    bucket's tail, one backward piece per cross layer;
  * captured into HIP graphs and replayed: the same bits as the eager step.
Reference: /root/reference/rec_now/layers/dcn_mix_layer.py:114-151, multi_dense_layer.py:80-94,
rec_block/pairwise_loss_from_batch.py:228-279."""
import os
import socket

import numpy as np
import pytest
import torch

import pairs_oracle as PO
from _chunked_oracle import GEMM_PRECISIONS, close, gemm_precision, run_chunked, weights64
from test_northstar_gpu import _mix_fwd, _randomise

pytestmark = pytest.mark.gpu


def _model(dev, B, D, S, N, L, seed, head_gain=40.0):
    from rec_now_amd.layers.dcn_mix_layer import DCNMixLayer
    from rec_now_amd.layers.multi_dense_layer import MultiDenseLayer
    torch.manual_seed(seed)                   # the layers' Glorot kernels come from torch's global generator: the same model in every run
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.7, (B, D)).astype(np.float32)
    groups = rng.integers(0, max(B // 64, 2), B).astype(np.float32)
    labels = (rng.random(B) < 0.25).astype(np.float32)
    cross, head = DCNMixLayer(S, num_layer=L, num_expert=N), MultiDenseLayer(1, 1)
    xd = torch.from_numpy(x).to(dev)
    head(cross(xd[:256]))
    _randomise(cross, seed + 1)
    with torch.no_grad():
        head.kernel.mul_(head_gain * (1024.0 / D) ** 0.5)      # scores of O(1): away from the softplus(0) = ln 2 plateau
        head.bias.fill_(0.3)
    return x, groups, labels, xd, torch.from_numpy(labels).to(dev), torch.from_numpy(groups).to(dev), cross, head


def _autograd_route(cross, head, xd, yd, gd, params):
    from rec_now_amd.fused import dcn_mix_score
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    for p in params:
        p.grad = None
    xr = xd.detach().clone().requires_grad_(True)
    scores = dcn_mix_score(cross, head, xr)
    loss, n_pair = pairwise_loss(scores, yd, gd, return_num_pair=True)
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().clone(), int(n_pair.item()), scores.detach().clone(), xr.grad.clone(), [p.grad.detach().clone() for p in params])


@pytest.mark.parametrize('B,D,S,N,L', [(2048, 256, 64, 2, 3), (512, 1024, 64, 2, 2), (1024, 128, 32, 4, 1)])
def test_step_equals_autograd_route_and_graph_replay(dev, B, D, S, N, L):
    from rec_now_amd.fused import score_params
    from rec_now_amd.step import DCNMixPairwiseStep
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 7 + B)
    params = score_params(cross, head)
    loss_a, np_a, sc_a, dx_a, g_a = _autograd_route(cross, head, xd, yd, gd, params)
    assert np_a > 0 and abs(float(loss_a) - np.log(2.0)) > 1e-3
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
    for mode in ('eager', 'graph'):
        if mode == 'graph':
            step.capture()
        for p in step.grads:
            p.fill_(float('nan'))
        step.dx.fill_(float('nan'))
        loss, n_pair = step.run() if mode == 'eager' else step.replay()
        torch.cuda.synchronize()
        assert int(n_pair.item()) == np_a, mode
        assert torch.equal(loss, loss_a) and torch.equal(step.scores, sc_a), mode
        assert torch.equal(step.dx, dx_a), mode
        for p, ga in zip(params, g_a):
            if p is head.bias:        # sum of dscores (0 in exact arithmetic): another summation order than the autograd route's column sum
                assert abs(float(p.grad) - float(ga)) <= 1e-5, (mode, float(p.grad), float(ga))
            else:
                assert torch.equal(p.grad, ga), (mode, tuple(p.shape))


def test_step_with_mask_and_wrong_order_pairs(dev):
    """mask and only_use_wrong_order_pair reach the loss stage as `pairwise_loss` passes them."""
    from rec_now_amd.fused import dcn_mix_score, score_params
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    from rec_now_amd.step import DCNMixPairwiseStep
    B, D, S, N, L = 1024, 256, 64, 2, 2
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 3)
    mask = torch.from_numpy(np.random.default_rng(5).random(B) < 0.8).to(dev)
    params = score_params(cross, head)
    for p in params:
        p.grad = None
    xr = xd.detach().clone().requires_grad_(True)
    loss_a = pairwise_loss(dcn_mix_score(cross, head, xr), yd, gd, only_use_wrong_order_pair=True, mask=mask)
    loss_a.backward()
    ref = [p.grad.detach().clone() for p in params]
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd, mask=mask, only_use_wrong_order_pair=True)
    loss, _ = step.run()
    torch.cuda.synchronize()
    assert torch.equal(loss, loss_a.detach()) and torch.equal(step.dx, xr.grad)
    for p, g in zip(params, ref):
        if p is not head.bias:
            assert torch.equal(p.grad, g)


@pytest.mark.parametrize('B,kind', [(4096, 'f32'), (9216, 'f32'), (9216, 'i32'), (16384, 'f32')])
def test_step_grouping_from_raw_ids_equals_the_two_call_form(dev, B, kind):
    """The step's GROUP phase forms canonical keys and solo flags INSIDE its grouping launch (k_front_small up to 8192 rows, k_front_mid<RAW> above:
    csrc/grouping.hip), with the row-block weight packs on the launch's other workgroups; `pairwise_loss` goes through recnow_group_keys +
    recnow_group_segments.  Ids with -0.0 / +0.0 (one group), NaN and +-inf (rows that pair with nobody: g_i - g_j is NaN in the reference,
    rec_block/pairwise_loss_from_batch.py:33-35) and negative values must give the same loss, pair count and gradients bit for bit."""
    from rec_now_amd.fused import score_params
    from rec_now_amd.step import DCNMixPairwiseStep
    D, S, N, L = 256, 64, 2, 2
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 21)
    rng = np.random.default_rng(22)
    if kind == 'f32':
        g = groups.copy()
        g[rng.integers(0, B, B // 16)] = -0.0
        g[rng.integers(0, B, B // 16)] = 0.0
        g[rng.integers(0, B, 40)] = np.nan
        g[rng.integers(0, B, 40)] = np.inf
        g[rng.integers(0, B, 40)] = -np.inf
        g[rng.integers(0, B, B // 8)] *= -1.0
        g[rng.integers(0, B, B // 8)] += 0.5
        gd = torch.from_numpy(g).to(dev)
    else:
        g = groups.astype(np.int32) - 7
        g[rng.integers(0, B, 50)] = np.iinfo(np.int32).min
        g[rng.integers(0, B, 50)] = np.iinfo(np.int32).max
        gd = torch.from_numpy(g).to(dev)
    params = score_params(cross, head)
    loss_a, n_a, scores_a, dx_a, grads_a = _autograd_route(cross, head, xd, yd, gd, params)
    assert n_a > 0
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
    for _ in range(2):                      # twice: the second step reuses every buffer (solo flags included)
        for p in params:
            p.grad = None
        loss, n_pair = step.run()
        torch.cuda.synchronize()
        assert int(n_pair.item()) == n_a and torch.equal(loss, loss_a)
        assert torch.equal(step.scores, scores_a) and torch.equal(step.dx, dx_a)
        for p, gr in zip(params, grads_a):
            if p is not head.bias:
                assert torch.equal(p.grad, gr)


@pytest.mark.parametrize('B', [4096, 12288])
def test_step_loss_walk_with_long_groups_equals_the_packed_form(dev, B):
    """The step's loss stage walks the pairs WITHOUT a pack launch (csrc/pairwise.hip k_pair_all<.., UNP>: a workgroup fills its LDS stage from scores /
    labels / mask through the sorted order), `pairwise_loss` on the packed member array.  A batch with one group beyond the 2048-member stage (its rows'
    walks gather per member), one long group that fits the stage (a wave per row) and many small ones, a mask on top: the same loss, pair count and
    gradients bit for bit (the arithmetic and its order are those of the packed form; /root/reference/rec_now/rec_block/pairwise_loss_from_batch.py:228-279)."""
    from rec_now_amd.fused import dcn_mix_score, score_params
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    from rec_now_amd.step import DCNMixPairwiseStep
    D, S, N, L = 256, 64, 2, 2
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 31)
    rng = np.random.default_rng(32)
    g = groups.copy()
    perm = rng.permutation(B)
    g[perm[:2500]] = 1.0e6          # > PW_STAGE members: never staged
    g[perm[2500:3200]] = 2.0e6      # > PW_LONG, fits the stage
    gd = torch.from_numpy(g).to(dev)
    mask = torch.from_numpy(rng.random(B) < 0.9).to(dev)
    params = score_params(cross, head)
    for p in params:
        p.grad = None
    xr = xd.detach().clone().requires_grad_(True)
    loss_a, n_a = pairwise_loss(dcn_mix_score(cross, head, xr), yd, gd, mask=mask, return_num_pair=True)
    loss_a.backward()
    ref = [p.grad.detach().clone() for p in params]
    assert int(n_a.item()) > 2500 * 100
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd, mask=mask)
    for _ in range(2):
        for p in params:
            p.grad = None
        loss, n_pair = step.run()
        torch.cuda.synchronize()
        assert int(n_pair.item()) == int(n_a.item()) and torch.equal(loss, loss_a.detach()) and torch.equal(step.dx, xr.grad)
        for p, gr in zip(params, ref):
            if p is not head.bias:
                assert torch.equal(p.grad, gr)


@pytest.fixture(scope='module')
def one_rank_rccl(dev):
    import torch.distributed as dist
    from rec_now_amd import dp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
    dist.init_process_group('nccl', device_id=dev)
    dp.FORCE_COLLECTIVES = True
    yield dist
    dp.FORCE_COLLECTIVES = False
    dist.destroy_process_group()


@pytest.mark.parametrize('B,two_streams,one_collective', [(8192, False, False), (8192, True, False), (8192, True, True), (16384, True, False), (32768, True, False),
                                                          (32768, True, True)])
def test_shard_sizes_through_reducer_vs_oracle(dev, one_rank_rccl, B, two_streams, one_collective):
    """(8192, 1024), (16 384, 1024) and (32 768, 1024): the 8-, 4- and 2-GPU shards of the metric's batch, step route + LayerwiseReducer over a 1-rank
    RCCL group (every collective runs), eager and replayed from graphs, against the fp64 oracle: loss, pair count, scores,
    d loss / d x and all 17 weight gradients."""
    from rec_now_amd import dp
    from rec_now_amd.fused import GpuEvent
    from rec_now_amd.step import DCNMixPairwiseStep
    D, S, N, L = 1024, 64, 2, 3
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 100 + B)
    stages = DCNMixPairwiseStep.stages_for(cross, head)
    # one_collective (RECNOW_DP_ONE_BUCKET=1): ONE all-reduce over all stages behind the last one -- the device path of the switch (waits on every stage's
    # event, both scale launches on the communication stream), same results as one collective per stage
    reducer = dp.LayerwiseReducer(stages, [GpuEvent() for _ in stages], dev, one_collective=one_collective)
    # two_streams: the eager step walks all layers in one call, weight-gradient products on a second stream, the library records the
    # stages' events (what bench.py runs under a process group); the replayed graphs are single-stream pieces either way
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd, reducer=reducer, two_streams=two_streams)
    named = dict(cross.named_weights())
    named['head/kernel'], named['head/bias'] = head.kernel, head.bias
    w64 = weights64(named)
    fwd = _mix_fwd(w64, L, head=True)
    (rs,), _, _ = run_chunked(fwd, torch.from_numpy(x), None, w64, chunk=4096, want_dx=False)
    rloss, rds, rP = PO.pairwise_bpr(groups, labels, rs.astype(np.float32))
    assert rP > B and abs(rloss - np.log(2.0)) > 1e-3
    _, rdx, rgrads = run_chunked(fwd, torch.from_numpy(x), torch.from_numpy(rds), w64, chunk=4096)
    # 'eager split': the same step with the split-precision products (at these sizes the product route: the row-block kernels are exact-fp32 only)
    for mode in ('eager', 'eager split', 'graph'):
        if mode == 'graph':
            step.capture()
        for f in reducer._flat:
            f.fill_(float('nan'))
        with gemm_precision('bf16x3' if mode == 'eager split' else 'f32'):
            loss, p_glob = step.replay() if mode == 'graph' else step.run()
            torch.cuda.synchronize()
        assert int(p_glob.item()) == rP and int(step.n_pair.item()) == rP, mode
        close(step.scores, rs, what='scores ' + mode)
        close(loss, np.float64(rloss), what='loss ' + mode)
        # d loss / d x is not a parameter: the reducer does not scale it (the loss SUM's gradient; bench.py does the same division)
        close(step.dx / (np.float32(rP) + np.float32(1e-10)), rdx, what='dx ' + mode)
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name + ' ' + mode, scale=np.abs(rds).sum() if name == 'head/bias' else None)


def test_step_route_at_the_metric_batch_vs_oracle(dev):
    """B = 65 536 x 1024, N = 1, no reducer: exactly the route `bench.py` times (whole-step entry, eager), outside bench.py -- loss, pair
    count, scores, d loss / d x and all 17 weight gradients against the fp64 chunked oracle + the C pair oracle (its segment-based form:
    the quadratic one takes minutes at this size; tests/test_oracle_golden.py holds the two forms together)."""
    from rec_now_amd.step import DCNMixPairwiseStep
    B, D, S, N, L = 65536, 1024, 64, 2, 3
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 4242)
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
    named = dict(cross.named_weights())
    named['head/kernel'], named['head/bias'] = head.kernel, head.bias
    w64 = weights64(named)
    fwd = _mix_fwd(w64, L, head=True)
    (rs,), _, _ = run_chunked(fwd, torch.from_numpy(x), None, w64, chunk=4096, want_dx=False)
    rloss, rds, rP = PO.pairwise_bpr(groups, labels, rs.astype(np.float32), grouped=True)
    assert rP > B and abs(rloss - np.log(2.0)) > 1e-3
    _, rdx, rgrads = run_chunked(fwd, torch.from_numpy(x), torch.from_numpy(rds), w64, chunk=4096)
    # the exact-fp32 products and the six-term split (bench.py's default at this size): one oracle, one bound; 'bf16x3 tile': the split-precision row-block
    # forward (RECNOW_TILE_SPLIT=1, csrc/dcnmix_tile_split.hip) in front of the split products' backward
    for prec in tuple(GEMM_PRECISIONS) + ('bf16x3 tile',):
        for f in step.grads:
            f.fill_(float('nan'))
        step.dx.fill_(float('nan'))
        tile = prec.endswith(' tile')
        if tile:
            os.environ['RECNOW_TILE_SPLIT'] = '1'
        try:
            with gemm_precision(prec.split()[0]):
                assert step.route_code() == (2 if tile else 0)
                loss, n_pair = step.run()
                torch.cuda.synchronize()
        finally:
            os.environ.pop('RECNOW_TILE_SPLIT', None)
        assert int(n_pair.item()) == rP
        close(step.scores, rs, what='scores ' + prec)
        close(loss, np.float64(rloss), what='loss ' + prec)
        close(step.dx, rdx, what='dx ' + prec)
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name + ' ' + prec, scale=np.abs(rds).sum() if name == 'head/bias' else None)


def test_backward_follows_what_its_forward_saved_when_the_precision_flips(dev):
    """B = 65 536: in split-precision mode the forward does not materialise x_{l+1} = x0 * O_l (csrc/dcnmix.hip `mix_xless`: the consumers form it in their
    operand loads), in exact mode it does.  The rule is read by the FORWARD; a backward issued after the switch was flipped must follow what its forward
    left in `saved` (the MIX_XLESS stamp), not the rule of the moment -- it would read a buffer nobody wrote.  Forward phases in one arithmetic, backward in
    the other, both orders, every gradient against the fp64 oracle."""
    from rec_now_amd.step import DCNMixPairwiseStep, _GROUP, _FORWARD, _LOSS, _BACKWARD
    B, D, S, N, L = 65536, 1024, 64, 2, 3
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 777)
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
    rs, rloss, rds, rP, rdx, rgrads, named = _oracle_step(x, groups, labels, cross, head, L)
    for fwd_prec, bwd_prec in (('bf16x3', 'f32'), ('f32', 'bf16x3')):
        for f in step.grads:
            f.fill_(float('nan'))
        step.dx.fill_(float('nan'))
        step._bind_grads()
        with gemm_precision(fwd_prec):
            step._call(_GROUP | _FORWARD | _LOSS)
        with gemm_precision(bwd_prec):
            step._call(_BACKWARD, L - 1, 0)
        torch.cuda.synchronize()
        what = fwd_prec + ' forward, ' + bwd_prec + ' backward'
        assert int(step.n_pair.item()) == rP
        close(step.scores, rs, what='scores, ' + what)
        close(step.dx, rdx, what='dx, ' + what)
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name + ', ' + what, scale=np.abs(rds).sum() if name == 'head/bias' else None)


def _oracle_step(x, groups, labels, cross, head, L, grouped=True):
    """fp64 chunked oracle of the layers + the C pair oracle: (scores, loss, d loss / d score, pairs, dx, {name: grad}, named weights)."""
    named = dict(cross.named_weights())
    named['head/kernel'], named['head/bias'] = head.kernel, head.bias
    w64 = weights64(named)
    fwd = _mix_fwd(w64, L, head=True)
    (rs,), _, _ = run_chunked(fwd, torch.from_numpy(x), None, w64, chunk=4096, want_dx=False)
    rloss, rds, rP = PO.pairwise_bpr(groups, labels, rs.astype(np.float32), grouped=grouped)
    _, rdx, rgrads = run_chunked(fwd, torch.from_numpy(x), torch.from_numpy(rds), w64, chunk=4096)
    return rs, rloss, rds, rP, rdx, rgrads, named


@pytest.mark.parametrize('B,reduced', [(8177, True), (16411, True), (65500, False)])
def test_ragged_batches_on_the_fast_route_vs_oracle(dev, one_rank_rccl, B, reduced):
    """The batches data parallelism really produces: whole groups per rank (dp.shard_rows_by_group), i.e. B % 256 != 0.  The step owns
    padded storage (recnow_dcn_mix_step_desc.B_pad: zero rows of x, zero d loss / d score) and runs the SAME kernels as a full batch --
    8177 and 16 411 rows on the row-block persistent kernels through the reducer over a 1-rank RCCL group, 65 500 rows on the
    launch-per-product route -- against the fp64 oracle of the B rows: loss, pair count, scores, d loss / d x, all 17 weight gradients.
    /root/reference/rec_now/rec_block/pairwise_loss_from_batch.py:254-279, layers/dcn_mix_layer.py:114-151."""
    from rec_now_amd import _lib, dp
    from rec_now_amd.fused import GpuEvent
    from rec_now_amd.step import DCNMixPairwiseStep
    D, S, N, L = 1024, 64, 2, 3
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 900 + B)
    reducer = None
    if reduced:
        stages = DCNMixPairwiseStep.stages_for(cross, head)
        reducer = dp.LayerwiseReducer(stages, [GpuEvent() for _ in stages], dev)
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd, reducer=reducer, two_streams=reduced)
    assert step.B == B and step.B_pad == -(-B // 256) * 256 and step.x.shape[0] == B and step.x.data_ptr() != xd.data_ptr()
    assert step.tile_route() == bool(_lib.load().recnow_dcn_mix_tile_route(step.B_pad, D, S, N, L)) == (B <= 16384)
    rs, rloss, rds, rP, rdx, rgrads, named = _oracle_step(x, groups, labels, cross, head, L)
    assert rP > B and abs(rloss - np.log(2.0)) > 1e-3
    for f in (reducer._flat if reduced else step.grads):
        f.fill_(float('nan'))
    step._dx_store.fill_(float('nan'))
    step._scores_store.fill_(float('nan'))
    for prec in GEMM_PRECISIONS:
        with gemm_precision(prec):
            for rep in range(2):                  # twice: the second step runs on the storage the first one left (padding rows still zero)
                loss, p_glob = step.run()
            torch.cuda.synchronize()
        assert int(p_glob.item()) == rP and int(step.n_pair.item()) == rP
        close(step.scores, rs, what='scores ' + prec)
        close(loss, np.float64(rloss), what='loss ' + prec)
        div = (np.float32(rP) + np.float32(1e-10)) if reduced else np.float32(1.0)      # under a reducer dx is the loss SUM's gradient
        close(step.dx / div, rdx, what='dx ' + prec)
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name + ' ' + prec, scale=np.abs(rds).sum() if name == 'head/bias' else None)
    # the padding: x rows stay zero, their dx is exactly zero, their scores are the head bias
    assert not step._x_store[B:].any() and not step._dx_store[B:].any()
    assert torch.equal(step._scores_store[B:], torch.full_like(step._scores_store[B:], float(head.bias.reshape(-1)[0])))


@pytest.mark.parametrize('B,D,L', [(100, 256, 2), (300, 512, 3), (1, 256, 1)])
def test_small_ragged_batches_through_the_step_vs_oracle(dev, B, D, L):
    """Batches below one 256-row block (down to a single row) through the step entry: padded to 256 / 512 rows, the grouping of the B rows in one
    launch from the raw ids, every gradient against the fp64 oracle; mask and integer ids ride along at B = 300."""
    from rec_now_amd.step import DCNMixPairwiseStep
    S, N = 64, 2
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, max(B, 256), D, S, N, L, 77 + B)
    x, groups, labels = x[:B], (groups[:B] % 7), labels[:B]
    xd, yd = xd[:B].contiguous(), yd[:B].contiguous()
    gd = torch.from_numpy(groups.astype(np.int32) if B == 300 else groups).to(dev)
    step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
    assert step.B == B and step.B_pad == -(-B // 256) * 256
    rs, rloss, rds, rP, rdx, rgrads, named = _oracle_step(x, groups, labels, cross, head, L, grouped=False)
    for _ in range(2):
        loss, n_pair = step.run()
    torch.cuda.synchronize()
    assert int(n_pair.item()) == rP
    # (a handful of scores: the bound is relative to the tensor's largest magnitude, and ONE score that happens to cancel to ~0.1 while its D
    #  terms are O(1) made this comparison fail once in a few runs with unseeded weights: scores are O(1) by construction, so that is the scale)
    close(step.scores, rs, what='scores', scale=max(float(np.abs(rs).max()), 1.0) if B < 32 else None)
    close(loss, np.float64(rloss), what='loss')
    if rP > 0:
        close(step.dx, rdx, what='dx')
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name, scale=np.abs(rds).sum() if name == 'head/bias' else None)
    else:
        assert not step.dx.any() and all(not p.grad.any() for p in named.values())
    assert not step._x_store[B:].any() and not step._dx_store[B:].any()


def test_ragged_batch_layer_routes_vs_oracle(dev):
    """B = 8177 through the drop-in routes: `head(cross(x))` + `pairwise_loss` as INTEGRATION.md writes it, and the fused node
    `dcn_mix_score`.  Both run the exact-128 formulation on a zero-padded copy (layers/_ops.py `ragged_pad_rows`); the same batch
    with the padding switched off (general kernels, leading dimension 160) is the third route.  All against the fp64 oracle."""
    from rec_now_amd.fused import dcn_mix_score, score_params
    from rec_now_amd.layers._ops import ragged_pad_rows
    from rec_now_amd.rec_block.pairwise_loss_from_batch import pairwise_loss
    B, D, S, N, L = 8177, 1024, 64, 2, 3
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 31)
    assert ragged_pad_rows(B, D, S, N, L) == 8192 and ragged_pad_rows(8192, D, S, N, L) == 0 and ragged_pad_rows(300, D, S, N, L) == 0
    rs, rloss, rds, rP, rdx, rgrads, named = _oracle_step(x, groups, labels, cross, head, L)
    params = score_params(cross, head)
    for route in ('drop-in', 'fused', 'drop-in unpadded'):
        if route == 'drop-in unpadded':
            os.environ['RECNOW_PAD_RAGGED'] = '0'
        try:
            for p in params:
                p.grad = None
            xr = xd.detach().clone().requires_grad_(True)
            scores = dcn_mix_score(cross, head, xr) if route == 'fused' else head(cross(xr)).reshape(-1)
            assert scores.shape == (B,)
            loss, n_pair = pairwise_loss(scores, yd, gd, return_num_pair=True)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            os.environ.pop('RECNOW_PAD_RAGGED', None)
        assert int(n_pair.item()) == rP, route
        close(scores, rs, what='scores ' + route)
        close(loss, np.float64(rloss), what='loss ' + route)
        assert xr.grad.shape == (B, D)
        close(xr.grad, rdx, what='dx ' + route)
        for name, p in named.items():
            close(p.grad, rgrads[name], what=name + ' ' + route, scale=np.abs(rds).sum() if name == 'head/bias' else None)


def test_gradient_accumulation_onto_bucket_views(dev):
    """dp.LayerwiseReducer + fused.dcn_mix_score(grad_buffers=...): a second backward without clearing the gradients must ADD to
    p.grad (= the bucket view), not overwrite it."""
    from rec_now_amd import dp
    from rec_now_amd.fused import GpuEvent, dcn_mix_score, score_params
    B, D, S, N, L = 512, 256, 64, 2, 2
    x, groups, labels, xd, yd, gd, cross, head = _model(dev, B, D, S, N, L, 11)
    params = score_params(cross, head)
    stages = [[p for p in params]]
    lw = dp.LayerwiseReducer(stages, [None], dev)
    gbuf = [lw.buffer_of(p) for p in params]
    gs = torch.randn(B, device=dev)
    for p in params:
        p.grad = None
    dcn_mix_score(cross, head, xd, grad_buffers=gbuf).backward(gs)
    torch.cuda.synchronize()
    once = [p.grad.detach().clone() for p in params]
    assert all(p.grad.data_ptr() == b.data_ptr() for p, b in zip(params, gbuf))
    dcn_mix_score(cross, head, xd, grad_buffers=gbuf).backward(gs)          # no clearing in between
    torch.cuda.synchronize()
    for p, g1 in zip(params, once):
        close(p.grad, 2.0 * g1, rtol=1e-6, what='accumulated gradient')


_TILE4096_CHILD = r'''
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests'); sys.path.insert(0, %(root)r + '/oracle')
from test_step_gpu import _model
from rec_now_amd.step import DCNMixPairwiseStep
dev = torch.device('cuda:0')
x, groups, labels, xd, yd, gd, cross, head = _model(dev, 16384, 256, 64, 2, 2, 77)
step = DCNMixPairwiseStep(cross, head, xd, yd, gd)
assert step.tile_route()
for _ in range(2):
    loss, n_pair = step.run()
torch.cuda.synchronize()
h = hashlib.sha256()
for t in [loss, step.scores, step.dx] + list(step.grads):
    h.update(t.detach().cpu().numpy().tobytes())
print('DIGEST', h.hexdigest(), int(n_pair.item()))
'''


def test_grouping_tile_without_a_front_kernel_does_not_mark_the_weight_packs_current(dev):
    """with RECNOW_GROUP_TILE=4096 the cooperative grouping of a 16 384-row shard runs WITHOUT the front kernel's pack workgroups;
    the GROUP phase must then not mark the row-block kernels' weight packs as written (the forward would skip its pack launch and run on stale or
    uninitialised packs).  Two child processes (the switches are read once per process): that setting against RECNOW_STEP_FRONT=0 (the pack as a launch
    of its own) -- loss, scores, d loss / d x and every gradient bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for extra in ({'RECNOW_GROUP_TILE': '4096'}, {'RECNOW_STEP_FRONT': '0'}):
        env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
        env.update(extra)
        out = subprocess.run([sys.executable, '-c', _TILE4096_CHILD % {'root': root}], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append([l for l in out.stdout.splitlines() if l.startswith('DIGEST')][-1])
    assert digests[0] == digests[1], digests

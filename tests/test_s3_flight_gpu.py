"""The four-set PAIR schedule of k_gemm_s3 (csrc/gemm_split.hip: a pair of k-tiles requested two pairs ahead, behind the B request of an even
k-tile) changes WHEN the A operands are requested, not what is summed in which order: every output -- C and the side columns -- has the bits of the
two-set schedule that RECNOW_S3_PAIR=0 routes to.  The switch is read once per process: one child process per setting, shared by all cases.

Which kernel a launch took is read from the profiler's kernel records of the child, not assumed: under the default setting every case must run
`k_gemm_s3<true, 0 | 1, true>` (the PAIR form), under RECNOW_S3_PAIR=0 `k_gemm_s3<true, 0 | 1, false>`, followed by the split-K reduce exactly where
the table says the product is split.

How each chunk length was obtained.  A k-tile is 16 k (SPL_BK).  The chunk is the launcher's (pick_split, csrc/gemm_dispatch.hpp): with M / 128 < 512 row
tiles the product is cut into s = min(ceil(512 / tiles), K / 256) slices of K / s; the split launcher wants K > 256.  So through recnow_gemm a chunk has at
least 16 k-tiles: 16 from a split K (K = 256 s), 20 and 24 from an unsplit K = 320 / 384 with few row tiles.  The PAIR loop is prologue, nt / 4 - 1 trips,
tail: 16 k-tiles are three trips + tail, i.e. the first trip behind the prologue, the steady state and the tail.  Chunks of exactly 4, 8 and 12 k-tiles
(tail only, one trip, two trips) cannot be launched through the library -- `_chunk` below restates the rule and the table is checked against it -- so
they are NOT covered here in isolation; the tail and the first trip run as part of every chunk."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, tb, mul, M, K, sp_r, slices, k-tiles per chunk).  N = 128; A is [M][K] with lda = K (a multiple of 32 floats) at the start of an allocation:
# rows on 128-byte lines.  tb = 0 is the GEMM1 layout (A alone), tb = 1 the dT2g layout (with and without A2).
CASES = [
    ('one_tile_unsplit_nt20', 0, 0, 128, 320, 2, 1, 20),
    ('one_tile_unsplit_mul_nt24', 1, 1, 128, 384, 1, 1, 24),
    ('two_tiles_split_mul_nt16', 1, 1, 256, 512, 2, 2, 16),
    ('two_tiles_split_nt16', 0, 0, 256, 1024, 1, 4, 16),
    ('one_tile_split_dt2g_nt16', 1, 0, 128, 768, 2, 3, 16),
    ('two_per_cu_split_mul_nt16', 1, 1, 8192, 2048, 2, 8, 16),      # 64 row tiles x 8 slices = 512 workgroups on 256 CUs
    ('two_per_cu_split_nt16', 0, 0, 8192, 2048, 1, 8, 16),
]


def _chunk(M, K):
    """(slices, k-tiles per chunk) of pick_split for a 128-column product with a side product."""
    tiles, s = M // 128, 1
    if tiles < 512:
        s = max(1, min(-(-512 // tiles), K // 256))
    kc = -(-(-(-K // s)) // 32) * 32
    return -(-K // kc), kc // 16


def run_cases():
    """Child-process entry: every case once under the profiler; prints the SHA of (C, Cx) per case and the k_gemm_s3 / reduce kernels in launch order."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from rec_now_amd import _lib
    from test_split_routes_gpu import _bound, _ref, run_longk
    dev = torch.device('cuda:0')
    _lib.call('recnow_set_gemm_precision', 1)
    sha = {}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i, (name, tb, mul, M, K, R, _, _) in enumerate(CASES):
            rng = np.random.default_rng(1000 + i)
            A = rng.standard_normal((M, K)).astype(np.float32)
            A2 = rng.uniform(-1, 1, (M, K)).astype(np.float32) if mul else None
            B = rng.standard_normal((K, 128)).astype(np.float32)
            Bx = rng.standard_normal((K, R)).astype(np.float32)
            C, Cx = run_longk(dev, 0, tb, A, A2, B, Bx)
            Rc, Rx, den, denx = _ref(A, A2, B, Bx)
            _bound(name + ' C', C, Rc, den)
            _bound(name + ' Cx', Cx, Rx, denx)
            sha[name] = hashlib.sha256(C.tobytes() + Cx.tobytes()).hexdigest()
        torch.cuda.synchronize()
    _lib.call('recnow_set_gemm_precision', 0)
    ev = sorted((e for e in prof.events() if 'k_gemm_s3' in e.name or 'k_gemm_splitk_reduce' in e.name), key=lambda e: e.time_range.start)
    print('RESULT ' + json.dumps({'sha': sha, 'kernels': [e.name for e in ev]}), flush=True)


_SNIPPET = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from test_s3_flight_gpu import run_cases
run_cases()
'''


@pytest.fixture(scope='module')
def children():
    out = {}
    for v in ('1', '0'):
        r = subprocess.run([sys.executable, '-c', _SNIPPET % (ROOT, os.path.join(ROOT, 'tests'))], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, RECNOW_S3_PAIR=v), cwd=ROOT)
        assert r.returncode == 0, 'child exit %d\n%s\n%s' % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        out[v] = json.loads([line for line in r.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])
    return out


def test_case_table_matches_the_launchers_chunk_rule():
    for name, _, _, M, K, _, s, nt in CASES:
        assert _chunk(M, K) == (s, nt), name
        assert nt % 4 == 0 and K % 32 == 0, name
    assert {c[7] for c in CASES} >= {16, 20, 24} and {c[6] for c in CASES} >= {1, 2}
    assert {(c[2], c[5]) for c in CASES} == {(0, 1), (0, 2), (1, 1), (1, 2)}          # A2 absent / present x one / two side columns
    assert any(c[3] // 128 * c[6] >= 512 for c in CASES)                              # two workgroups on each of 256 CUs


def _kernel_form(name):
    """('s3', A2K, PAIR) of a k_gemm_s3 record, ('reduce',) of the split-K reduce."""
    if 'k_gemm_splitk_reduce' in name:
        return ('reduce',)
    args = name[name.index('k_gemm_s3<') + len('k_gemm_s3<'):].split('>')[0].replace(' ', '').split(',')
    assert args[0] == 'true', name
    return ('s3', int(args[1]), len(args) > 2 and args[2] in ('true', '1'))


def test_every_case_took_the_kernel_it_is_about(children):
    for v, pair in (('1', True), ('0', False)):
        want = []
        for _, _, mul, _, _, _, s, _ in CASES:
            want.append(('s3', mul, pair))
            if s > 1:
                want.append(('reduce',))
        got = [_kernel_form(n) for n in children[v]['kernels']]
        assert got == want, 'RECNOW_S3_PAIR=%s: %r' % (v, children[v]['kernels'])


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_pair_schedule_has_the_bits_of_the_two_set_schedule(children, name):
    assert children['1']['sha'][name] == children['0']['sha'][name]

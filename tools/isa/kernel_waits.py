"""The vector-memory wait counts of a kernel's steady-state loop (device-only compile to assembly, as kernel_regs.py).

    python tools/isa/kernel_waits.py rec_now_amd/csrc/gemm_split.hip [name-filter, default k_gemm_s3] [-DRN_...]

For every kernel whose name (demangled where llvm-cxxfilt is installed) contains the filter: the backward-branch loop that holds the most MFMAs, written as one line of events in program order:
    m<n>   n MFMAs                      L<n>   n global loads requested
    vm<n>  s_waitcnt vmcnt(n)           |      s_barrier
vmcnt retires in order: `L8 ... vm3` lets the three youngest loads stay in flight, `vm0` waits for every load requested so far.
Reads the `s_waitcnt vmcnt` / `global_load` / `v_mfma` / `s_barrier` / branch lines of the project's own assembly, nothing else.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CXXFILT = shutil.which('llvm-cxxfilt') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'llvm-cxxfilt')


def loop_events(lines):
    """(first, last) line of the loop with the most MFMAs of one function body and its event string."""
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r'(\.LBB\d+_\d+):', ln)] if m}
    loops = []
    for i, ln in enumerate(lines):
        b = re.match(r'\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)', ln)
        if b and labels.get(b.group(1), i) < i:
            loops.append((labels[b.group(1)], i))
    if not loops:
        return None, ''
    a, b = max(loops, key=lambda x: sum('v_mfma' in ln for ln in lines[x[0]:x[1]]))
    ev, loads, mfma = [], 0, 0

    def flush():
        nonlocal loads, mfma
        if mfma:
            ev.append('m%d' % mfma)
        if loads:
            ev.append('L%d' % loads)
        loads = mfma = 0

    for ln in lines[a:b]:
        op = ln.split(';')[0]
        if 'global_load' in op:
            if mfma:
                flush()
            loads += 1
        elif 'v_mfma' in op:
            if loads:
                flush()
            mfma += 1
        w = re.search(r's_waitcnt[^;]*vmcnt\((\d+)\)', op)
        if w or 's_barrier' in op:
            flush()
            ev.append('vm%s' % w.group(1) if w else '|')
    flush()
    return (a, b), ' '.join(ev)


def main():
    src = sys.argv[1]
    rest = sys.argv[2:]
    filt = rest.pop(0) if rest and not rest[0].startswith('-') else 'k_gemm_s3'
    out = src if src.endswith('.s') else os.path.join(tempfile.mkdtemp(), 'k.s')          # a .s file: assembly of this project made before
    if out != src:
        subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-function', '--cuda-device-only', '-S', src, '-o', out,
                        '-I' + os.path.join(ROOT, 'include')] + rest, check=True, stderr=subprocess.DEVNULL)
    txt = open(out).read()
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        name = m.group(1)
        try:
            name = subprocess.run([CXXFILT, name], capture_output=True, text=True).stdout.strip() or name
        except OSError:
            pass
        if filt not in name:
            continue
        span, ev = loop_events(m.group(2).split('\n'))
        print('%s\n    loop of %s lines: %s' % (name[:110], span[1] - span[0] if span else 0, ev))


if __name__ == '__main__':
    main()

"""Register figures and per-basic-block instruction mix of k_segw<13, 3> (csrc/wrap_kernels.hpp), from the gfx950 assembly.

Compiles a translation unit that instantiates the kernel (device only, -S, the library's flags) and prints arch VGPRs, AGPRs and
scratch, then per basic block the counts of MFMA, other VALU, v_accvgpr_read / _write, SALU, VMEM, s_waitcnt and s_nop, and the longest
run of MFMAs with nothing between them.  Needs hipcc, no GPU.

usage: python tools/segw_asm_report.py [--csrc DIR] [--min N] [--keep FILE.s] [--plain] [extra hipcc flags ...]
  --csrc DIR   the directory holding wrap_kernels.hpp (default: pycusdr_amd/csrc of this tree; point it at another checkout to compare)
  --min N      leave out blocks of fewer than N instructions (default 8)
  --keep F     also write the assembly to F
  --plain      without -mllvm -amdgpu-mfma-vgpr-form (the library's compile line has it since round 13: the MFMAs write arch VGPRs)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TU = '#include "wrap_kernels.hpp"\ntemplate __global__ void k_segw<13, 3>(SegWArgs);\n'
COLS = ('mfma', 'valu', 'acc_read', 'acc_write', 'salu', 'vmem', 'lds', 'waitcnt', 'nop', 'other')


def classify(op):
    if op.startswith('v_mfma') or op.startswith('v_smfma'):
        return 'mfma'
    if op.startswith('v_accvgpr_read'):
        return 'acc_read'
    if op.startswith('v_accvgpr_write'):
        return 'acc_write'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('ds_'):
        return 'lds'
    if op == 's_waitcnt':
        return 'waitcnt'
    if op == 's_nop':
        return 'nop'
    if op.startswith('s_'):
        return 'salu'
    return 'other'


def report(asm, min_insts):
    m = re.search(r'\n(_Z\w*k_segw\w*):[^\n]*\n(.*?)\n\s*s_endpgm', asm, re.S)
    if not m:
        sys.exit('no k_segw in the assembly')
    name, body = m.group(1), m.group(2)

    def figure(pattern):
        v = re.search(pattern, asm[m.end():])
        return int(v.group(1)) if v else None

    arch = figure(r'\.amdhsa_accum_offset\s+(\d+)')          # where the AGPRs begin: the arch VGPRs the kernel is given
    agpr = figure(re.escape(name) + r'\.num_agpr,\s*(\d+)')
    sgpr = figure(re.escape(name) + r'\.numbered_sgpr,\s*(\d+)')
    scratch = figure(re.escape(name) + r'\.private_seg_size,\s*(\d+)')
    total = figure(r'\.vgpr_count:\s+(\d+)')
    spill = figure(r'\.vgpr_spill_count:\s+(\d+)')
    occ = figure(r'; Occupancy:\s+(\d+)')
    print(f'== {name}')
    print(f'arch VGPRs {arch} (accum_offset)  AGPRs {agpr}  VGPR + AGPR allocated {total}  SGPRs {sgpr}  '
          f'scratch {scratch} B  spilled VGPRs {spill}  waves per SIMD (compiler) {occ}')
    print(f'{"block":14s} {"insts":>6s} ' + ' '.join(f'{c:>9s}' for c in COLS) + f' {"v_pk_*":>7s} {"mfma_run":>8s}')
    label, cnt, pk, run, best = 'entry', collections.Counter(), 0, 0, 0

    def flush():
        tot = sum(cnt.values())
        if tot >= min_insts:
            print(f'{label:14s} {tot:6d} ' + ' '.join(f'{cnt[c]:9d}' for c in COLS) + f' {pk:7d} {best:8d}')

    for line in body.split('\n'):
        lm = re.match(r'^(\.LBB[\d_]+):', line) or re.match(r'^; (%bb\.\d+):', line)      # a fall-through block has a comment only
        if lm:
            flush()
            label, cnt, pk, run, best = lm.group(1), collections.Counter(), 0, 0, 0
            continue
        im = re.match(r'^\s+([a-z][a-z_0-9]*)(\s|$)', line)
        if not im:
            continue
        kind = classify(im.group(1))
        cnt[kind] += 1
        if im.group(1).startswith('v_pk_'):
            pk += 1
        if kind == 'mfma':
            run += 1
            best = max(best, run)
        else:
            run = 0
    flush()


def main(argv):
    csrc, min_insts, keep, extra, form = os.path.join(ROOT, 'pycusdr_amd', 'csrc'), 8, None, [], ['-mllvm', '-amdgpu-mfma-vgpr-form']
    i = 0
    while i < len(argv):
        if argv[i] == '--csrc':
            csrc = os.path.abspath(argv[i + 1]); i += 2
        elif argv[i] == '--min':
            min_insts = int(argv[i + 1]); i += 2
        elif argv[i] == '--keep':
            keep = argv[i + 1]; i += 2
        elif argv[i] == '--plain':
            form = []; i += 1
        else:
            extra.append(argv[i]); i += 1
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, 'segw_tu.hip'), os.path.join(d, 'segw_tu.s')
        with open(src, 'w') as f:
            f.write(TU)
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S', '-I', csrc] + form + extra + ['-o', out, src]
        subprocess.check_call(cmd)
        asm = open(out).read()
    if keep:
        with open(keep, 'w') as f:
            f.write(asm)
    report(asm, min_insts)


if __name__ == '__main__':
    main(sys.argv[1:])

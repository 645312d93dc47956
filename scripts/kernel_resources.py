#!/usr/bin/env python3
"""Register / spill / LDS / occupancy table of every kernel of the given .hip files (CPU-side cross compile for
gfx950, the flags of scripts/kernel_regs.sh plus the per-file ones of build.py), as JSON on stdout:

    scripts/kernel_resources.py [--csrc DIR] amt_flac.hip amt_png.hip ...  > side.json
    scripts/kernel_resources.py --join parent.json tree.json > both.json     # {kernel: {parent, tree}}, differing first
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (('vgpr', r'\bVGPRs'), ('agpr', r'AGPRs'), ('sgpr', r'TotalSGPRs'), ('vgpr_spill', r'VGPRs Spill'),
          ('sgpr_spill', r'SGPRs Spill'), ('scratch_bytes_per_lane', r'ScratchSize \[bytes/lane\]'),
          ('lds_bytes', r'LDS Size \[bytes/block\]'), ('occupancy_waves_per_simd', r'Occupancy \[waves/SIMD\]'))


def resources(csrc, names):
    spec = importlib.util.spec_from_file_location('amt_build', os.path.join(ROOT, 'amt-saga_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    flags = [f for f in b.FLAGS if not f.startswith('-I') and f not in ('-Wall', '-Wno-unused-function')]
    table = {}
    for name in names:
        cmd = [b.HIPCC] + flags + b.FILE_FLAGS.get(name, []) + ['-I' + os.path.join(ROOT, 'include'), '-I' + csrc, '-c',
               os.path.join(csrc, name), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage']
        out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        for block in out.split('Function Name: ')[1:]:
            kernel = subprocess.run(['c++filt', block.split()[0]], capture_output=True, text=True).stdout.strip()
            kernel = re.sub(r'\(.*', '', kernel)
            table[name + ':' + kernel] = {k: int(re.search(pat + r': (\d+)', block).group(1)) for k, pat in FIELDS}
    return table


def main(argv):
    if argv and argv[0] == '--join':
        parent, tree = (json.load(open(p)) for p in argv[1:3])
        both = {k: dict(parent=parent.get(k), tree=tree.get(k)) for k in sorted(set(parent) | set(tree))}
        order = sorted(both, key=lambda k: both[k]['parent'] == both[k]['tree'])
        print(json.dumps({k: both[k] for k in order}, indent=1))
        return
    csrc = os.path.join(ROOT, 'amt-saga_amd', 'csrc')
    if argv and argv[0] == '--csrc':
        csrc, argv = os.path.abspath(argv[1]), argv[2:]
    print(json.dumps(resources(csrc, argv), indent=1))


if __name__ == '__main__':
    main(sys.argv[1:])

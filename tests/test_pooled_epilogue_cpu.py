"""CPU: the W-pooled epilogue forms of the two FFT-domain row kernels (EPI = 5) keep two workgroups on a CU -- at most 128
VGPRs and no scratch memory, under the flags the library is built with (hipcc cross-compiles without a GPU)."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_module():
    spec = importlib.util.spec_from_file_location('amt_build', os.path.join(ROOT, 'amt-saga_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pooled_row_kernels_fit_two_workgroups_per_cu():
    b = _build_module()
    if not os.path.exists(b.HIPCC):
        pytest.skip('hipcc not available')
    procs = []
    for src, kernel in (('amt_fftconv.hip', 'fc_row_kernelILb1ELi5E'), ('amt_fftpk.hip', 'pk_row_kernelILb1ELi5E')):
        cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(src, []) + ['-c', os.path.join(b.CSRC, src), '-o', os.devnull,
                                                                 '-Rpass-analysis=kernel-resource-usage']
        procs.append((kernel, subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True)))
    for kernel, p in procs:
        out = p.communicate()[1]
        assert p.returncode == 0, out[-2000:]
        blocks = [blk for blk in out.split('Function Name: ')[1:] if kernel in blk.split()[0]]
        assert len(blocks) == 1, kernel
        blk = blocks[0]
        vgpr = int(re.search(r'\bVGPRs: (\d+)', blk).group(1))
        spill = int(re.search(r'VGPRs Spill: (\d+)', blk).group(1))
        scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', blk).group(1))
        occ = int(re.search(r'Occupancy \[waves/SIMD\]: (\d+)', blk).group(1))
        assert vgpr <= 128 and spill == 0 and scratch == 0 and occ >= 4, (kernel, vgpr, spill, scratch, occ)

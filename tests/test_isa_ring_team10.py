"""Static check of the weight ring in the constant-team-size form of the packed policy kernel (CPU only: hipcc
cross-compiles gfx950 without a GPU).  Dropping units of the first packed layer moves the ring's refills to another unit
of the same tap and makes one copy of the layer per wave: every path must still load, wait for and use each of the
stream's items exactly once, in 256 VGPRs at two waves per SIMD, with no more scratch than the run-time-N form."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_team10_kernels_keep_the_ring_discipline(tmp_path):
    import check_ring_isa
    from gnn_pathplanning_amd._native import RING_KERNELS, RING_KERNELS_TEAM
    # (the ISA _native.build() kept is the code that ships when it is at least as new as every source: as tests/test_isa_ring.py)
    csrc = os.path.join(ROOT, 'gnn_pathplanning_amd', 'csrc')
    kept = os.path.join(ROOT, 'gnn_pathplanning_amd', 'build', 'product', 'gnnpp_api-hip-amdgcn-amd-amdhsa-gfx950.s')
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc))
    newest = max(newest, os.path.getmtime(os.path.join(ROOT, 'include', 'gnnpp.h')))
    if os.path.exists(kept) and os.path.getmtime(kept) >= newest:
        out = kept
    else:
        out = str(tmp_path / 'gnnpp.s')
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                               '-Wno-unused-result', '-w', os.path.join(csrc, 'gnnpp_api.hip'), '-o', out])
    assert [k[1] for k in RING_KERNELS_TEAM] == [342, 366, 390]              # 294 + 24 K items, K = 2, 3, 4
    runtime_n = {k[1]: k for k in RING_KERNELS if 'ILb1E' in k[0] and 'ELb1ELi0E' in k[0]}
    for kern, items, scratch in RING_KERNELS_TEAM:
        errors, stats, meta = check_ring_isa.check(out, kern, scratch)
        assert not errors, (kern, errors[:10])
        assert stats['loads'] == items and stats['takes'] == items, (kern, stats)
        assert meta['NumVgprs'] == 256 and meta['Occupancy'] == 2, (kern, meta)
        _, _, meta0 = check_ring_isa.check(out, runtime_n[items][0], scratch)
        assert meta['ScratchSize'] <= meta0['ScratchSize'], (kern, meta, meta0)   # scratch did not grow

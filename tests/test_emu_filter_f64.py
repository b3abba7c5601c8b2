"""CPU: the graph-filter kernels against float64 on the host emulation (tests/emu/) -- a reduced version of
tests/test_gpu_filter_f64.py's matrix (same runner, same yardstick, small B).  The split-f16 cases at input scales
1e-3 and 1e-6 are the ones an unscaled hi / lo split of z fails: its lo halves are f16 subnormals there, an absolute
error floor of ~2^-25 |w| per product (1e-2 relative at 1e-6)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

import filter_f64_cases as fc  # noqa: E402
from gnn_pathplanning_amd._native import (TUNE_FILTER_GPW, TUNE_FILTER_PIPE_GRID, TUNE_FILTER_SMALL,
                                          TUNE_FILTER_SMALL_ROWS, TUNE_FILTER_SPLIT)  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


LSIGF = [
    # lsigf_kernel<RTW 1, NW 8, NG 8, H2 under split-f16>: one graph of 12 nodes per workgroup, batched S
    dict(name='lsigf<rtw1,nw8,ng8>/B2N12K3', seed=1, B=2, N=12, G=128, F=128, K=3, E=1, bias='feat'),
    # <RTW 2, NW 16>: two graphs of 12 per workgroup; node-major x and y, ReLU, fp64 S
    dict(name='lsigf<rtw2,nw16,ng8>/gpw2/nodemajor/relu/f64S', seed=2, B=3, N=12, G=128, F=128, K=2, E=1,
         bias='feat', x_nm=1, y_nm=1, relu=1, f64=1, knobs={TUNE_FILTER_GPW: 2}),
    # run-time NG (G = 33), F = 129 in two chunks with a per-node bias, Nin < N, shared S, E = 2
    dict(name='lsigf<ng-runtime>/G33F129/pernode/Nin<N/sharedS/E2', seed=3, B=2, N=9, Nin=6, G=33, F=129, K=2, E=2,
         bias='node', batched=False),
    # nsplit = 2 forced over a 40-node graph (3 row tiles), S view offset by one float (s_vec4 off), K = 5
    dict(name='lsigf<nsplit2>/N40K5/s_offset', seed=4, B=3, N=40, G=128, F=128, K=5, E=1, s_offset=1,
         knobs={TUNE_FILTER_SPLIT: 2}),
    # the training form: tap signals kept (gnnpp_lsigf_fwd_save), E = 2, F = 64 (MTP 4)
    dict(name='lsigf_save<rtw1,nw8,ng8>/E2F64', seed=5, B=2, N=10, G=128, F=64, K=3, E=2, bias='feat', save=True),
    # taps spread over 1e-3 .. 1e2
    dict(name='lsigf<rtw1,nw8,ng8>/tap_spread', seed=6, B=2, N=10, G=128, F=128, K=4, E=1, tap_spread=True),
    # N = 1 (no neighbours), K = 1
    dict(name='lsigf<rtw1,nw8,ng8>/N1K1', seed=7, B=5, N=1, G=128, F=128, K=1, E=1, bias='feat'),
    # lsigf_small_b3_kernel (FILTER_SMALL = 2, 32-row workgroups; other precisions: lsigf_kernel), ragged last group
    dict(name='small_b3<rows32>/N5/ragged', seed=8, B=9, N=5, G=128, F=128, K=3, E=1, bias='feat', x_nm=1, y_nm=1,
         knobs={TUNE_FILTER_SMALL: 2, TUNE_FILTER_SMALL_ROWS: 32}),
    # lsigf_pipe_b3_kernel (FILTER_SMALL = 3, persistent grid of 7)
    dict(name='pipe_b3<grid7>/N4', seed=9, B=40, N=4, G=128, F=128, K=2, E=1, bias='feat', x_nm=1, y_nm=1,
         knobs={TUNE_FILTER_SMALL: 3, TUNE_FILTER_PIPE_GRID: 7}),
]


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', LSIGF, ids=lambda c: c['name'])
def test_emu_lsigf_f64(bk, case, prec, scale):
    fc.run_lsigf(bk, case, prec, scale)


HEAD = [
    # policy_filter_kernel: split-f16 -> mode 0, fp32 MFMA -> 1, bf16x3 -> 2 (own plane buffer)
    dict(name='policy_filter/N20K3', seed=11, B=2, N=20, K=3, modes={0: 2, 1: 1, 2: 0}),
    # K = 2: the last shift writes hi | lo directly; fp64 S
    dict(name='policy_filter/N33K2/f64S', seed=12, B=1, N=33, K=2, f64=1, modes={0: 2, 1: 1, 2: 0}),
    # K = 4: a conversion pass between shifts; unaligned S
    dict(name='policy_filter/N17K4/s_offset', seed=13, B=2, N=17, K=4, s_offset=1, modes={0: 2, 1: 1, 2: 0}),
]


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', fc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', HEAD, ids=lambda c: c['name'])
def test_emu_filter_head_f64(bk, case, prec, scale):
    fc.run_head(bk, case, prec, scale)


@pytest.mark.parametrize('scale', (1e-6, 1.0))
@pytest.mark.parametrize('masked', (0, 1))
def test_emu_input_grad_f64(bk, masked, scale):
    c = dict(name='input_grad/N12K3', seed=21, B=2, N=12, G=128, F=128, K=3, E=1, x_nm=1)
    fc.run_input_grad(bk, c, scale, masked)
    if not masked:
        fc.run_input_grad(bk, dict(c, x_nm=0, name='input_grad/featmajor/E2', E=2), scale, masked)

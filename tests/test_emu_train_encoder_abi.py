"""CPU: the train-mode encoder's C entry points (csrc/train_encoder.hip, compiled unmodified for the host emulation) on
poisoned workspaces between guards -- a reduced matrix of tests/train_encoder_abi_cases.py (which says what a case
checks): the shapes (1, 1), (3, 7) and (10, 13) under 0 and 16 weight-gradient workgroups, (1, 2) and (2, 3) under 100.
A write outside gnnpp_encoder_train_workspace_floats(N, B) or a read of workspace nobody wrote shows here, on host memory,
before the same case runs on a device (tests/test_gpu_train_encoder_abi.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

import filter_f64_cases as fc  # noqa: E402
import train_encoder_abi_cases as ab  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('case', ab.EMU_CASES, ids=ab.case_id)
def test_emu_train_encoder_abi(bk, case):
    ab.run_case(bk, case)


def test_emu_knobs_are_restored(bk):
    """run_case leaves both training knobs as it found them, also when the case fails inside."""
    from gnn_pathplanning_amd import _native
    keys = (_native.TUNE_TRAIN_WGRAD_WGS, _native.TUNE_TRAIN_RUNNING_FUSED)
    before = [bk.lib.gnnpp_get_tuning(k) for k in keys]
    assert before == [0, 1]
    case = dict(next(c for c in ab.CASES if c['shape'] == (1, 1) and c['wgs'] == 16), N=0)   # N = 0: refused by the call
    with pytest.raises(AssertionError):
        ab.run_case(bk, case)
    assert [bk.lib.gnnpp_get_tuning(k) for k in keys] == before

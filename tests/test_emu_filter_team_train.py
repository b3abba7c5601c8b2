"""CPU: the training calls of the team filter on neighbour lists (gnnpp_team_lists_transpose,
gnnpp_lsigf_team_lists_fwd_save, gnnpp_lsigf_team_lists_input_grad) on the host emulation: the byte equalities
include/gnnpp.h states, every result against float64, the error tables.  Cases and runner:
tests/filter_team_train_cases.py (a reduced matrix; tests/test_gpu_filter_team_train.py runs all of it)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import filter_team_cases as tc  # noqa: E402
import filter_team_train_cases as tt  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('case', tt.TRANSPOSE_CASES, ids=lambda c: c['name'])
def test_emu_lists_transpose(bk, case):
    tt.run_transpose(bk, case)


def test_emu_lists_transpose_errors(bk):
    tt.run_transpose_errors(bk)


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', tt.EMU_FILTER_CASES, ids=lambda c: c['name'])
def test_emu_forward_keeps_tap_signals(bk, case, prec):
    tt.run_save(bk, case, prec)


@pytest.mark.parametrize('case', tt.EMU_FILTER_CASES, ids=lambda c: c['name'])
def test_emu_input_grad_is_the_filter_on_the_transposed_lists(bk, case):
    tt.run_input_grad(bk, case)


def test_emu_train_call_errors(bk):
    tt.run_train_errors(bk)

"""CPU: the five launches of csrc/train_ops.hip (gnnpp_gemm_kmajor, gnnpp_gemm_kmajor_multi, gnnpp_linear_fwd,
gnnpp_policy_loss, gnnpp_adam_step) on the host emulation, through the C ABI: every result against a float64 statement
(f64_yardstick), the bytes around every output, two calls the same bytes, the error tables.  Cases and runners:
tests/train_ops_cases.py (a reduced matrix: without K = 5120 and B N = 3000; tests/test_gpu_train_ops.py runs all of
it).  In addition to tests/test_emu_training.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import train_ops_cases as to  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')
by_name = lambda c: c['name']                                               # noqa: E731


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


def test_emu_gemm_plan_is_the_library_s(bk):
    to.run_gemm_plan(bk, to.GEMM_CASES + to.GPU_GEMM_CASES + to.MULTI_CASES)


@pytest.mark.parametrize('case', to.EMU_GEMM_CASES, ids=by_name)
def test_emu_gemm_kmajor_against_float64(bk, case):
    to.run_gemm(bk, case)


def test_emu_gemm_multi_is_each_product_alone(bk):
    to.run_gemm_multi(bk)


def test_emu_gemm_refusals(bk):
    to.run_gemm_errors(bk)


@pytest.mark.parametrize('case', to.EMU_LINEAR_CASES, ids=by_name)
def test_emu_linear_fwd_against_float64(bk, case):
    to.run_linear(bk, case)


def test_emu_linear_fwd_relu_at_exactly_zero(bk):
    to.run_linear_relu_zero(bk)


def test_emu_linear_fwd_refusals(bk):
    to.run_linear_errors(bk)


@pytest.mark.parametrize('case', to.EMU_LOSS_CASES, ids=by_name)
def test_emu_policy_loss_against_float64(bk, case):
    to.run_loss(bk, case)


def test_emu_policy_loss_refusals(bk):
    to.run_loss_errors(bk)


@pytest.mark.parametrize('case', to.EMU_ADAM_CASES, ids=by_name)
def test_emu_adam_step_against_float64(bk, case):
    to.run_adam(bk, case)


def test_emu_adam_step_refusals(bk):
    to.run_adam_errors(bk)

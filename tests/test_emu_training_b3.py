"""CPU: the train-mode encoder with its convolutions on bf16x3 planes (csrc/train_encoder_b3.hip: conv_b3_kernel, compiled
unmodified for the host emulation) through gnnpp_encoder_train_fwd_prec / _bwd_prec at B = 3, N = 2 -- ragged image chunks
of every geometry -- on poisoned workspaces and packs, against the float64 statement with the unchanged fp32 yardstick
(tests/train_b3_cases.py); and the exact-fp32 value of the new calls against the existing pair, byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

import filter_f64_cases as fc  # noqa: E402
import train_b3_cases as b3  # noqa: E402
import train_encoder_abi_cases as ab  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


def test_emu_b3_training_against_float64(bk):
    b3.run_poisoned(bk, N=2, B=3, seed=2003)


def test_emu_option_off_is_the_parent(bk):
    N, B = 2, 3
    sd, obs, cot = ab.inputs(N, B, 2003, False)
    obs_np, cot_np = obs.numpy(), np.ascontiguousarray(cot.permute(1, 0, 2).numpy())
    nan = ab.POISONS[1][1]
    old, _, _, ws_old = b3.call_once(bk, N, B, sd, obs_np, cot_np, nan, 'old')
    new, _, _, ws_new = b3.call_once(bk, N, B, sd, obs_np, cot_np, nan, 'fp32')
    assert ab._flat(old) == ab._flat(new)
    assert np.array_equal(ws_old, ws_new)                     # every float of the workspace, written or not

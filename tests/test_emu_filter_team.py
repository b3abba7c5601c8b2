"""CPU: the team graph filter (graphs of up to 1024 nodes spread over workgroups: csrc/lsigf_team_kernel.hip) on the
host emulation of tests/emu/, against float64 with the fp32 numpy statement as the yardstick (runner:
tests/filter_team_cases.py; statements, inputs and yardstick: tests/filter_f64_cases.py, unchanged).

Small B, both supported precisions (GNNPP_PREC_FP32 = bf16x3, GNNPP_PREC_FP32_MFMA), the four input scales.  Covered:
N = 113, 130, 200 (not a multiple of 16), 257 and one case at N = 40 (the call is not tied to large N); K = 1 .. 4;
E = 1, 2; G / F = 128 / 128, 48 / 40, 33 / 128; no bias, per feature, per node; S float and double, batched and shared,
unsymmetric and symmetric, one full and one empty column; the head variant; the error table; the version; determinism."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

import filter_f64_cases as fc  # noqa: E402
import filter_team_cases as tc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


TEAM = [
    dict(name='team/N113K3/feat', seed=1, B=2, N=113, G=128, F=128, K=3, E=1, bias='feat'),
    dict(name='team/N130K2E2/G48F40/node/sharedS/f64S', seed=2, B=2, N=130, G=48, F=40, K=2, E=2, bias='node',
         batched=False, f64=1),
    dict(name='team/N200K4/G33F128/nobias/relu/full_empty', seed=3, B=1, N=200, G=33, F=128, K=4, E=1, relu=1,
         s='full_empty'),
    dict(name='team/N257K1/feat/nullS', seed=4, B=1, N=257, G=128, F=128, K=1, E=1, bias='feat', null_s=True),
    dict(name='team/N257K3/G48F40/sym/f64S', seed=5, B=1, N=257, G=48, F=40, K=3, E=1, bias='feat', s='sym', f64=1),
    dict(name='team/N40K3/feat/relu', seed=6, B=2, N=40, G=128, F=128, K=3, E=1, bias='feat', relu=1),
    dict(name='team/N113K4E2/G33F128/node/sharedS', seed=7, B=2, N=113, G=33, F=128, K=4, E=2, bias='node',
         batched=False, s='full_empty'),
    dict(name='team/N130K3/unsym/nobias', seed=8, B=1, N=130, G=128, F=128, K=3, E=1, s='unsym'),
]

HEAD = [
    dict(name='team/N130K3/feat', seed=11, B=2, N=130, G=128, F=128, K=3, E=1, bias='feat'),
    dict(name='team/N200K2/G48F40/f64S/full_empty', seed=12, B=1, N=200, G=48, F=40, K=2, E=1, bias='feat', f64=1,
         s='full_empty'),
    dict(name='team/N113K1E2/G33F128/nobias', seed=13, B=2, N=113, G=33, F=128, K=1, E=2),
    dict(name='team/N40K4', seed=14, B=1, N=40, G=128, F=128, K=4, E=1, bias='feat'),
]


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', TEAM, ids=lambda c: c['name'])
def test_emu_team_lsigf_f64(bk, case, prec, scale):
    tc.run_team(bk, case, prec, scale)


@pytest.mark.parametrize('scale', fc.SCALES)
@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', HEAD, ids=lambda c: c['name'])
def test_emu_team_head_f64(bk, case, prec, scale):
    tc.run_team_head(bk, case, prec, scale)


def test_emu_team_errors(bk):
    tc.run_errors(bk)


def test_emu_team_version(bk):
    assert bk.lib.gnnpp_version() == 330


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
def test_emu_team_deterministic(bk, prec):
    tc.run_team(bk, TEAM[0], prec, 1.0, twice=True)
    tc.run_team(bk, TEAM[6], prec, 1.0, twice=True)

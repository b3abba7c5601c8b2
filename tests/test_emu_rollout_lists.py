"""CPU: gnnpp_rollout_lists (csrc/rollout_team_lists_kernel.hip, compiled unmodified for the host emulation): the
communication graph as the team filter's neighbour lists, against the lists of the oracle's dense S and against
gnnpp_team_lists_from_dense of gnnpp_rollout_gso's S, bit for bit; radius and connected against both.  Instances and
runner: tests/rollout_lists_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import rollout_lists_cases as lc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('case', lc.CASES, ids=lambda c: c['name'])
def test_emu_rollout_lists(bk, case):
    lc.run_lists_case(bk, case)


def test_emu_rollout_lists_errors(bk):
    lc.run_lists_errors(bk)

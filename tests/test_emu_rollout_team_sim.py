"""CPU: the large-team simulator kernels (csrc/rollout_team_kernels.hip, csrc/rollout_team_lists_kernel.hip, compiled
unmodified for the host emulation) at their map and team-size edges -- non-square maps, maps inside the field of view, the
three map-load paths of observe_stage at N = 129, the team sizes at the kernels' seams, dense teams at either end of the
range, hand-built graph states -- and every graph kernel, the one-wave ones included, on the thin maps (1 x 65 536,
65 536 x 1) where a squared distance passes 2^31, against the sequential oracle, bit for bit.  Instances:
tests/rollout_team_sim_cases.py; runners: tests/rollout_sim_cases.py and tests/rollout_lists_cases.py.  The launchers' LDS
requests run on the device only (tests/test_gpu_rollout_team_sim_cases.py): the emulation grants any LDS size."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import rollout_lists_cases as lc  # noqa: E402
import rollout_sim_cases as sc  # noqa: E402
import rollout_team_sim_cases as tsc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('case', tsc.all_cases(), ids=lambda c: c['name'])
def test_emu_rollout_team_sim(bk, case):
    sc.run_case(bk, case)


def test_emu_rollout_team_sim_map_load_paths(bk):
    """With the pointers the calls are really given, the map-load cases reach all three paths of observe_stage."""
    paths = set()
    for case in tsc.map_load_cases():
        paths |= set(sc.load_paths(case, sc.SimState(bk, case).g['grid'].ptr))
    assert paths == {1, 4, 16}


@pytest.mark.parametrize('case', tsc.lists_cases(), ids=lambda c: c['name'])
def test_emu_rollout_team_sim_lists(bk, case):
    lc.run_lists_case(bk, case)

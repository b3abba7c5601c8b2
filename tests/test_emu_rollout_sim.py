"""CPU: the one-wave simulator kernels (csrc/rollout_kernels.hip, compiled unmodified for the host emulation) at their map
and team-size edges: non-square maps, maps inside the field of view, the three map-load paths of observe_stage, the team
sizes at the kernels' seams and hand-built graph states through the fused launches, against the sequential oracle, bit
for bit.  Instances and runner: tests/rollout_sim_cases.py.  The launchers' LDS branches and gnnpp_rollout_policy_step
run on the device only (tests/test_gpu_rollout_sim_cases.py): the emulation grants any LDS size, and the fused policy
kernel is too slow under it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import rollout_sim_cases as sc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('case', sc.all_cases(), ids=lambda c: c['name'])
def test_emu_rollout_sim(bk, case):
    sc.run_case(bk, case)


def test_emu_rollout_sim_map_load_paths(bk):
    """With the pointers the calls are really given, the map-load cases reach all three paths of observe_stage."""
    paths = set()
    for case in sc.map_load_cases():
        paths |= set(sc.load_paths(case, sc.SimState(bk, case).g['grid'].ptr))
    assert paths == {1, 4, 16}

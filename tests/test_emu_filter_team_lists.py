"""CPU: the team filter on caller-provided neighbour lists (gnnpp_lsigf_team_lists_fwd, gnnpp_filter_head_team_lists_fwd,
gnnpp_policy_team_lists_fwd) on the host emulation: bit-identical to the dense-S team calls on the S the lists were made
from (gnnpp_team_lists_from_dense), the error table, and the Python helpers' numpy restatement of the block.  Cases
and runner: tests/rollout_lists_cases.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_f64_cases as fc  # noqa: E402
import filter_team_cases as tc  # noqa: E402
import rollout_lists_cases as lc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists('/opt/rocm/lib/llvm/bin/clang++'),
                                reason='host clang++ from ROCm not present')


@pytest.fixture(scope='module')
def bk():
    import emu_lib
    return fc.EmuBackend(emu_lib.load())


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', lc.FILTER_CASES, ids=lambda c: c['name'])
def test_emu_filter_lists_equal_dense(bk, case, prec):
    lc.run_filter_equal(bk, case, prec)


def test_emu_policy_lists_equal_dense(bk):
    # (8 agents: the emulated encoder is the cost of this test; the GPU file runs N = 20, 130 and 1024)
    lc.run_policy_equal(bk, 1, 8, 2, 0, seed=42)


def test_emu_filter_lists_errors(bk):
    lc.run_filter_errors(bk)


def test_emu_lists_from_dense_is_the_columns_of_s(bk):
    """gnnpp_team_lists_from_dense against numpy: per column the ascending non-zero rows of S and their weights (fp64
    rounded like S.float()), a full and an empty column, the padding."""
    import numpy as np
    for c in (lc.FILTER_CASES[1], lc.FILTER_CASES[3], lc.FILTER_CASES[5]):
        _, S, _, _ = fc.make_inputs(c['seed'], c['B'], c['N'], c['G'], c['F'], c['K'], c['E'], None,
                                    c.get('batched', True))
        S = lc._s_variant(c, S)
        blk = lc.filter_lists(bk, S, c['N'])
        lc.check_block(c['name'], blk.get(), lc.lists_of_dense(S.astype(np.float32).reshape(-1, c['N'], c['N'])))

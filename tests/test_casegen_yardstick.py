"""CPU, no library: the yardstick of gnnpp_casegen (tests/casegen_cases.py) on every named case -- each case shows what
its name says (its facts), and the yardstick's own answer has the properties rules 2-5 of include/gnnpp_casegen.h
guarantee: distinct starts, distinct goals, no agent on its own goal, everything inside one connected free region, and a
grid that is the raw map plus filled cells."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import casegen_cases as cc  # noqa: E402


@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_yardstick_answers_have_the_contract_properties(name):
    want = cc.wants_of(name)
    cc.assert_properties(want)
    assert set(np.unique(want['status']).tolist()) <= {cc.OK, cc.TOO_SMALL}


def test_the_named_cases_cover_ok_and_too_small():
    status = np.concatenate([cc.wants_of(n)['status'] for n in cc.EMU_CASES])
    assert (status == cc.OK).any() and (status == cc.TOO_SMALL).any()


def test_property_check_sees_a_broken_answer():
    """The check must fail on an answer that breaks a rule, or it would prove nothing."""
    want = {k: v.copy() for k, v in cc.wants_of('random_20x20').items()}
    want['goal'][3, 0] = want['start'][3, 0]
    with pytest.raises(AssertionError):
        cc.assert_properties(want)
    want = {k: v.copy() for k, v in cc.wants_of('equal_components_keep_the_lowest_cell').items()}
    want['grid'][0, :, 4:6] = 0                           # a second free component
    with pytest.raises(AssertionError):
        cc.assert_properties(want)


def test_threshold_of_density():
    assert cc.threshold_of(0) == 0 and cc.threshold_of(1.0) == 2 ** 32 - 1 and cc.threshold_of(0.5) == 2 ** 31

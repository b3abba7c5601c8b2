"""GPU (-m gpu): the train-mode encoder's C entry points on the MI355X, on poisoned workspaces between guards -- the whole
matrix of tests/train_encoder_abi_cases.py (which says what a case checks): both feature layouts, train_pack NULL and the
caller's, update_running 0 and 1, 0 / 16 / 100 / 2048 weight-gradient workgroups, the running statistics fused and in a
launch of their own, at six shapes against float64, and 10 x 129 (the 256-workgroup side of the weight-gradient switch)
for guards and poisons alone.  And the Python door's hold on GNNPP_TUNE_TRAIN_WGRAD_WGS between a forward and its
backward (decentralplanner._EncoderTrainFunction)."""
import pytest
import torch

import filter_f64_cases as fc
import train_encoder_abi_cases as ab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


@pytest.mark.parametrize('case', ab.CASES, ids=ab.case_id)
def test_train_encoder_abi_against_float64(bk, case):
    ab.run_case(bk, case)


@pytest.mark.parametrize('case', ab.GUARD_ONLY, ids=ab.case_id)
def test_train_encoder_abi_guards_at_the_workgroup_switch(bk, case):
    ab.run_case(bk, case)


def _planner(dev, sd, N):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from test_gpu_training_f64 import Cfg
    net = DecentralPlannerNet(Cfg(N, 3, dev)).to(dev)
    net.load_state_dict(sd)
    net.train()
    return net


def _encoder_loss(net, obs, cot):
    """A scalar of the train-mode encoder's features alone (DecentralPlannerNet._train_encoder: the autograd function
    over all agents), so that the backward pass holds the encoder's node and nothing else."""
    return (net._train_encoder(obs) * cot).sum()


def test_backward_refuses_a_changed_wgrad_knob(dev):
    """Forward under GNNPP_TUNE_TRAIN_WGRAD_WGS = 0, knob set to 16, backward(): GnnppError naming both values BEFORE any
    launch (under 16 workgroups the weight-gradient kernels would address partial slabs the forward's workspace does not
    hold), and every parameter's .grad is still None.  With the knob back at 0, a fresh forward and backward gives the
    bits of a twin that was never disturbed: features, all 20 gradients, running statistics, counters."""
    from gnn_pathplanning_amd import _native
    from test_gpu_training_f64 import make_case
    L = _native.lib()
    B, N = 7, 3
    sd, obs, _, _ = make_case(B, N, seed=77)
    obs = obs.to(dev)
    cot = torch.randn(B, N, 128, generator=torch.Generator().manual_seed(78)).to(dev)
    assert L.gnnpp_get_tuning(_native.TUNE_TRAIN_WGRAD_WGS) == 0
    twin = _planner(dev, sd, N)
    twin_loss = _encoder_loss(twin, obs, cot)
    twin_loss.backward()
    torch.cuda.synchronize()
    net = _planner(dev, sd, N)
    loss = _encoder_loss(net, obs, cot)
    try:
        assert L.gnnpp_set_tuning(_native.TUNE_TRAIN_WGRAD_WGS, 16) == 0
        with pytest.raises(_native.GnnppError) as err:
            loss.backward()
        assert 'is 16' in str(err.value) and 'under 0' in str(err.value)
    finally:
        assert L.gnnpp_set_tuning(_native.TUNE_TRAIN_WGRAD_WGS, 0) == 0
    torch.cuda.synchronize()
    assert all(p.grad is None for p in net.parameters())
    # knob back at 0: a fresh forward and backward of a fresh planner
    net2 = _planner(dev, sd, N)
    loss2 = _encoder_loss(net2, obs, cot)
    loss2.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss2.detach(), twin_loss.detach())
    for (k, p), (_, q) in zip(net2.named_parameters(), twin.named_parameters()):
        if k.startswith('ConvLayers.'):
            assert p.grad is not None and torch.equal(p.grad, q.grad), k
        else:
            assert p.grad is None and q.grad is None, k
    for (k, a), (_, b) in zip(net2.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), k
    assert int(net2.ConvLayers[1].num_batches_tracked) == N

"""GPU: the packed one-plane pixel image + patch-fed first-layer stream of the bf16x3 encoder against the three-plane
word path of the same library (GNNPP_TUNE_ENCODER_ONE_PLANE = 0 routes every tile through b3_l0_generic, which
multiplies the same non-zero products in the same order): the logits of forward() must be torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pathplanning_amd._native import TUNE_ENCODER_ONE_PLANE as ONE_PLANE  # noqa: E402


def _pixels(kind, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'binary':
        return (torch.rand(B, N, 3, 11, 11, generator=g) < 0.3).float()
    x = torch.randn(B, N, 3, 11, 11, generator=g) * 3.0
    x = (x.view(torch.int32) & -65536).view(torch.float32)               # exactly one bf16 each, both signs
    x[torch.rand(x.shape, generator=g) < 0.2] = 0.0
    return x


def _gso(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(B, N, N, generator=g) * (torch.rand(B, N, N, generator=g) < min(1.0, 6.0 / N))
    S = (S + S.transpose(1, 2)) * 0.2
    S.diagonal(dim1=1, dim2=2).zero_()
    return S.contiguous()


@pytest.mark.parametrize('kind', ['binary', 'bf16'])
@pytest.mark.parametrize('B,N', [(512, 10), (256, 50), (128, 100), (37, 7)], ids=['c2', 'c3', 'c5', 'ragged'])
def test_packed_l0_logits_equal_word_path(kind, B, N):
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    from oracle import policy_oracle as orc
    dev = torch.device('cuda:0')
    L = _native.lib()

    class Cfg:
        num_agents, nGraphFilterTaps, device = N, 3, dev
    net = DecentralPlannerNet(Cfg()).to(dev).eval()
    net.load_state_dict(orc.init_state_dict(3))
    obs = _pixels(kind, B, N, seed=B + N).to(dev)
    net.addGSO(_gso(B, N, seed=N).to(dev))
    out = []
    assert L.gnnpp_get_tuning(ONE_PLANE) == 1
    for knob in (1, 0):
        assert L.gnnpp_set_tuning(ONE_PLANE, knob) == 0
        try:
            with torch.no_grad():
                lg = torch.stack(list(net(obs)))                         # forward(): one [B, 5] block per agent
            torch.cuda.synchronize()
        finally:
            L.gnnpp_set_tuning(ONE_PLANE, 1)
        out.append(lg.cpu().clone())
    assert out[0].shape == (N, B, 5)
    assert torch.isfinite(out[0]).all() and out[0].abs().max() > 0
    assert torch.equal(out[0], out[1])

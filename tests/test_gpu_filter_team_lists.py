"""GPU (-m gpu): the team filter on caller-provided neighbour lists on the MI355X: bit-identical to the dense-S team
calls (the cases of tests/test_emu_filter_team_lists.py plus 2 x 1024 nodes), the error table, and the Python layer:
graphML.team_lists_* helpers and lsigf_team(lists=...).  Cases and runner: tests/rollout_lists_cases.py."""
import numpy as np
import pytest
import torch

import filter_f64_cases as fc
import filter_team_cases as tc
import rollout_lists_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def bk(dev):
    from gnn_pathplanning_amd import _native
    return fc.TorchBackend(_native.lib(), dev)


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('case', lc.FILTER_CASES + lc.GPU_FILTER_CASES, ids=lambda c: c['name'])
def test_filter_lists_equal_dense(bk, case, prec):
    lc.run_filter_equal(bk, case, prec)


@pytest.mark.parametrize('prec', tc.PRECS, ids=fc.PREC_NAMES.get)
@pytest.mark.parametrize('shape', [(2, 20, 1), (2, 130, 2), (1, 130, 4), (2, 1024, 3)], ids=str)
def test_policy_lists_equal_dense(bk, shape, prec):
    B, N, K = shape
    lc.run_policy_equal(bk, B, N, K, prec, seed=50 + N + K, s='full_empty' if K == 4 else None)


def test_filter_lists_errors(bk):
    lc.run_filter_errors(bk)


def test_lists_from_dense_is_the_columns_of_s(bk):
    for c in (lc.FILTER_CASES[1], lc.FILTER_CASES[3], lc.FILTER_CASES[5]):
        _, S, _, _ = fc.make_inputs(c['seed'], c['B'], c['N'], c['G'], c['F'], c['K'], c['E'], None,
                                    c.get('batched', True))
        S = lc._s_variant(c, S)
        blk = lc.filter_lists(bk, S, c['N'])
        lc.check_block(c['name'], blk.get(), lc.lists_of_dense(S.astype(np.float32).reshape(-1, c['N'], c['N'])))


def _dense(dev, seed, B, E, N, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    S = (torch.rand(B, E, N, N, generator=g) < 0.1) * torch.rand(B, E, N, N, generator=g)
    S[..., :, 3] = 0.5                                   # a full column
    S[..., :, 5] = 0                                     # an empty one
    return S.to(dtype).to(dev)


def test_python_helpers_round_trip(dev):
    """team_lists_to_dense(team_lists_from_dense(S)) == S.float(); views and sizes; a bad block raises."""
    from gnn_pathplanning_amd import _native, graphML as gml
    for dtype, shape in ((torch.float32, (2, 1, 20, 20)), (torch.float64, (2, 2, 130, 130)), (torch.float32, (1, 17, 17))):
        S = _dense(dev, 3, shape[0], shape[1] if len(shape) == 4 else 1, shape[-1], dtype=dtype).reshape(shape)
        N = shape[-1]
        graphs = S.numel() // (N * N)
        blk = gml.team_lists_from_dense(S)
        assert blk.dtype is torch.uint8 and blk.numel() == gml.team_lists_bytes(graphs, N) == lc.layout(graphs, N)[3]
        cnt, idx, val = gml.team_lists_views(blk, graphs, N)
        assert cnt.shape == (graphs, N) and idx.shape == val.shape == (graphs, N, (N + 3) & ~3)
        assert cnt.dtype is torch.int32 and idx.dtype is torch.uint16 and val.dtype is torch.float32
        assert torch.equal(cnt.reshape(S.shape[:-2] + (N,)).long(), (S.float() != 0).sum(-2))
        back = gml.team_lists_to_dense(blk, graphs, N)
        assert back.shape == (graphs, N, N) and torch.equal(back, S.float().reshape(graphs, N, N))
    assert gml.team_lists_bytes(0, 5) == 0 and gml.team_lists_bytes(1, 1025) == 0
    S = _dense(dev, 4, 1, 1, 20)
    blk = gml.team_lists_from_dense(S)
    cnt, idx, val = gml.team_lists_views(blk, 1, 20)
    bad = blk.clone()
    gml.team_lists_views(bad, 1, 20)[1].view(torch.int16)[0, 3, 1] = 20                      # an index >= N
    with pytest.raises(_native.GnnppError):
        gml.team_lists_to_dense(bad, 1, 20)
    bad = blk.clone()
    gml.team_lists_views(bad, 1, 20)[0][0, 7] = 21                         # a count > N
    with pytest.raises(_native.GnnppError):
        gml.team_lists_to_dense(bad, 1, 20)
    bad = blk.clone()
    gml.team_lists_views(bad, 1, 20)[0][0, 7] = -1
    with pytest.raises(_native.GnnppError):
        gml.team_lists_to_dense(bad, 1, 20)
    with pytest.raises(_native.GnnppError):
        gml.team_lists_views(blk[:-16], 1, 20)                            # too small


@pytest.mark.parametrize('prec', ['fp32', 'fp32_mfma'])
def test_lsigf_team_lists_keyword(dev, prec):
    """graphML.lsigf_team(lists=block) == lsigf_team(S), shared and batched S; S and lists together are refused."""
    from gnn_pathplanning_amd import _native, graphML as gml
    B, E, N, G, F, K = 2, 2, 130, 48, 40, 3
    g = torch.Generator().manual_seed(8)
    h = (torch.randn(F, E, K, G, generator=g) / (G * K * E) ** 0.5).to(dev)
    x = torch.randn(B, N, G, generator=g).to(dev)
    b = torch.randn(F, 1, generator=g).to(dev)
    for S in (_dense(dev, 9, B, E, N), _dense(dev, 10, 1, E, N)[0]):
        want = gml.lsigf_team(h, S, x, b, relu=True, precision=prec)
        got = gml.lsigf_team(h, None, x, b, relu=True, precision=prec, lists=gml.team_lists_from_dense(S),
                             batched=S.dim() == 4)
        assert torch.equal(want, got)
    with pytest.raises(_native.GnnppError):
        gml.lsigf_team(h, S, x, b, lists=gml.team_lists_from_dense(S))
    with pytest.raises(_native.GnnppError):
        gml.lsigf_team(h, None, x, b)

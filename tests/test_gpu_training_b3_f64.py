"""GPU (-m gpu): the training step with trainPrecision='bf16x3' (the train-mode encoder's forward and input-gradient
convolutions on bf16x3 planes, csrc/train_encoder_b3.hip) against the float64 statement of the same step.

The claim under test is "fp32-equivalent", so the bf16x3 path is held to what any fp32 implementation is held to: the
statement, the scaffolding and the scales of tests/test_gpu_training_f64.py and the yardstick of tests/f64_yardstick.py
(RMS_K, MAX_K, ULPS), all imported unmodified -- the same statement run by torch in fp32 on the CPU measures what fp32
arithmetic costs; no margin of the path's own is added.  Compared: loss, logits, encoder features, every parameter
gradient, running mean / variance, num_batches_tracked and the parameters after one FusedAdam step.

Shapes: B = 1, N = 1 (one image: every chunk partial), 3 x 2 (no multiple of the 2- and 4-image chunks of the 11x11 and 5x5
layers), 33 x 2 (one image past the 32-image chunk of the dense layers), 64 x 3 (full chunks); {0, 1} observations and
real-valued ones (normal values times 2^k, k per channel from -20 .. 20); and 3 x 2 with layer 0's convolution weights
scaled by 2^-40 and layer 2's by 2^30.  Then determinism, the exact-fp32 value of the new C calls against the existing pair
byte for byte, GraphedTrainStep, train_step_lists at N = 130, a frozen encoder and FlatBucketDP."""
import numpy as np
import pytest
import torch

import test_gpu_training_f64 as t64
from f64_yardstick import ULP, ULPS, gap                                           # noqa: F401  (the unchanged yardstick)
from test_gpu_training_f64 import check_adam, check_against_f64, dev, make_case, run_planner, statement  # noqa: F401

pytestmark = pytest.mark.gpu

ADAM = (1e-3, 1e-5, None)


class CfgB3(t64.Cfg):
    """test_gpu_training_f64.Cfg + the config field under test."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.trainPrecision = 'bf16x3'


@pytest.fixture
def b3(monkeypatch):
    """Every planner the imported scaffolding builds carries trainPrecision='bf16x3', and every train-mode encoder call is
    seen to run with a b3 pack (a test that silently took the fp32 path would prove nothing)."""
    from gnn_pathplanning_amd import decentralplanner as dp
    calls = []
    orig = dp.DecentralPlannerNet._train_pack_b3
    monkeypatch.setattr(t64, 'Cfg', CfgB3)
    monkeypatch.setattr(dp.DecentralPlannerNet, '_train_pack_b3',
                        lambda self, tensors: (calls.append(1), orig(self, tensors))[1])
    yield calls
    assert calls, 'no train-mode encoder call asked for the bf16x3 pack'


def scaled_obs(sd, B, N, seed):
    """Real-valued observations: normal values times 2^k, k drawn per channel from -20 .. 20, without max-pool near-ties."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-20, 21, (3,), generator=g)
    scale = (2.0 ** k.double()).float().reshape(3, 1, 1)
    draw = lambda *shape: torch.randn(*shape, generator=g) * scale                  # noqa: E731
    return t64.without_pool_near_ties(sd, draw(B, N, 3, 11, 11), draw)


def one_b3_case(dev, monkeypatch, B, N, seed, kind):
    sd, obs, S, tgt = make_case(B, N, seed=seed, margin=False)
    if kind == 'real':
        obs = scaled_obs(sd, B, N, seed + 5)
    elif kind == 'wscale':
        sd['ConvLayers.0.weight'] = sd['ConvLayers.0.weight'] * 2.0 ** -40
        sd['ConvLayers.7.weight'] = sd['ConvLayers.7.weight'] * 2.0 ** 30
    w64 = statement(sd, S, obs, tgt, N, torch.float64)
    w32 = statement(sd, S, obs, tgt, N, torch.float32)
    got = run_planner(dev, sd, obs, S, tgt, N, 3, 1, 1, True, monkeypatch, ADAM)
    assert set(got['grads']) == set(w64['grads']) == set(w32['grads'])
    bad = check_against_f64(got, w64, w32, B, N) + check_adam(sd, got, ADAM)
    assert not bad, '\n'.join(str(b) for b in bad)
    return got


@pytest.mark.parametrize('kind', ['binary', 'real'])
@pytest.mark.parametrize('B,N', [(1, 1), (3, 2), (33, 2), (64, 3)])
def test_b3_training_step_against_float64(dev, monkeypatch, b3, B, N, kind):
    one_b3_case(dev, monkeypatch, B, N, 7000 + 10 * B + N, kind)


def test_b3_scaled_weights_against_float64(dev, monkeypatch, b3):
    """Layer 0's convolution weights x 2^-40, layer 2's x 2^30 at B = 3, N = 2: the exponent range a split-f16 operand loses."""
    one_b3_case(dev, monkeypatch, 3, 2, 7032, 'wscale')


def _encoder_pass(dev, sd, obs, cot, N):
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    net = DecentralPlannerNet(CfgB3(N, 3, dev)).to(dev)
    net.load_state_dict(sd)
    net.train()
    feat = net._train_encoder(obs)
    (feat * cot).sum().backward()
    torch.cuda.synchronize()
    return [feat.detach().cpu()] + [p.grad.cpu() for k, p in net.named_parameters() if k.startswith('ConvLayers.')] + \
        [b.cpu() for k, b in net.named_buffers() if 'running' in k]


def test_b3_is_deterministic(dev, b3):
    """Two identical steps (fresh planners, fresh workspaces): byte-identical features, gradients, running statistics."""
    B, N = 33, 2
    sd, obs, _, _ = make_case(B, N, seed=91, margin=False)
    cot = torch.randn(B, N, 128, generator=torch.Generator().manual_seed(92)).to(dev)
    a = _encoder_pass(dev, sd, obs.to(dev), cot, N)
    b = _encoder_pass(dev, sd, obs.to(dev), cot, N)
    assert len(a) == 1 + 20 + 10
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()


def test_option_off_is_the_parent(dev):
    """gnnpp_encoder_train_fwd_prec / _bwd_prec with GNNPP_PREC_FP32_MFMA and pack_b3 = NULL against gnnpp_encoder_train_fwd /
    _bwd on the same inputs and NaN-filled workspaces: byte-identical features, gradients, running statistics, counters --
    and workspaces (every float, written or not)."""
    import filter_f64_cases as fc
    import train_b3_cases as cases
    import train_encoder_abi_cases as ab
    from gnn_pathplanning_amd import _native
    bk = fc.TorchBackend(_native.lib(), dev)
    N, B = 3, 7
    sd, obs, cot = ab.inputs(N, B, 3007, False)
    obs_np, cot_np = obs.numpy(), np.ascontiguousarray(cot.permute(1, 0, 2).numpy())
    nan = ab.POISONS[1][1]
    old, _, _, ws_old = cases.call_once(bk, N, B, sd, obs_np, cot_np, nan, 'old')
    new, _, _, ws_new = cases.call_once(bk, N, B, sd, obs_np, cot_np, nan, 'fp32')
    assert ab._flat(old) == ab._flat(new)
    assert np.array_equal(ws_old, ws_new)
    # and the bf16x3 value is another arithmetic: the same step is NOT the parent's bytes
    b3run, _, _, _ = cases.call_once(bk, N, B, sd, obs_np, cot_np, nan, 'bf16x3')
    assert ab._flat(b3run) != ab._flat(old)


def test_b3_graphed_step_replays_the_eager_steps(dev, b3):
    """GraphedTrainStep with trainPrecision='bf16x3': after its three eager warm-up steps, three replays leave the bytes of
    three eager steps (the b3 pack is rebuilt inside the captured step, behind the optimizer)."""
    from gnn_pathplanning_amd import training as tr
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    B, N = 8, 4
    batches, sd = [], None
    for seed in (8403, 8413, 8423, 8433):
        sd_i, obs, S, tgt = make_case(B, N, seed=seed, margin=False)
        sd = sd or sd_i
        batches.append((obs.to(dev), tgt.to(dev), S.to(dev)))
    results = []
    for graphed in (False, True):
        net = DecentralPlannerNet(CfgB3(N, 3, dev)).to(dev)
        net.load_state_dict(sd)
        net.train()
        opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
        if graphed:
            step = tr.GraphedTrainStep(net, opt, *batches[0])        # (3 eager warm-up steps, then the capture)
            for b in batches[1:]:
                step(*b)
        else:
            for b in [batches[0]] * 3 + batches[1:]:
                tr.train_step(net, opt, *b)
        torch.cuda.synchronize()
        results.append({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
        if k.startswith('ConvLayers.') and k.endswith('weight'):
            assert not torch.equal(results[1][k], sd[k]), k


def test_b3_train_step_lists_against_float64(dev, monkeypatch, b3):
    """train_step_lists at N = 130, B = 2 (the large-team route: neighbour lists of the graph) with the bf16x3 encoder."""
    from gnn_pathplanning_amd import decentralplanner as dp, graphML as gml, training as tr
    B, N = 2, 130
    sd, obs, S, tgt = make_case(B, N, seed=21300, margin=False)
    w64 = statement(sd, S, obs, tgt, N, torch.float64)
    w32 = statement(sd, S, obs, tgt, N, torch.float32)
    net = dp.DecentralPlannerNet(CfgB3(N, 3, dev)).to(dev)
    net.load_state_dict(sd)
    net.train()
    seen = {}
    orig, orig_loss = dp._EncoderTrainFunction.apply, tr._policy_loss_and_grad
    with monkeypatch.context() as mp:
        mp.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('feat', orig(*a)))
        mp.setattr(tr, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg), orig_loss(lg, t))[1])
        opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
        lists = gml.team_lists_from_dense(S.to(dev).unsqueeze(1))
        loss = tr.train_step_lists(net, opt, obs.to(dev), tgt.to(dev), lists, symmetric=False)
    torch.cuda.synchronize()
    got = dict(loss=loss.cpu(), feat=seen['feat'].detach().cpu(), logits=seen['logits'].detach().permute(1, 0, 2).cpu(),
               grads={k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()},
               params={k: p.detach().cpu().clone() for k, p in net.named_parameters()},
               running={k: b.detach().cpu().clone() for k, b in net.named_buffers() if 'running' in k},
               nbt={k: int(b) for k, b in net.named_buffers() if 'num_batches' in k})
    bad = check_against_f64(got, w64, w32, B, N) + check_adam(sd, got, ADAM)
    assert not bad, '\n'.join(str(b) for b in bad)


def test_b3_frozen_encoder_against_float64(dev, monkeypatch, b3):
    """tests/train_freeze_cases.py style: the `direct` route with the whole encoder frozen, and with its BatchNorm scales
    and shifts frozen, through train_step -- frozen tensors get no gradient and keep their bytes, the others meet the
    yardstick."""
    import train_freeze_cases as fc
    from gnn_pathplanning_amd import decentralplanner as dp, training as tr
    r = 'direct'
    c = fc.ROUTES[r]
    sd, obs, S, tgt = fc.build(r)
    w64, w32 = fc.statements(r)
    for pattern in ('encoder_frozen', 'bn_affine_frozen'):
        net = fc.freeze(fc.planner(r, dev), pattern)
        net.trainPrecision = 'bf16x3'                          # (fc.planner's config has no such field: set on the planner)
        opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
        seen = {}
        orig, orig_loss = dp._EncoderTrainFunction.apply, tr._policy_loss_and_grad
        with monkeypatch.context() as mp:
            mp.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('feat', orig(*a)))
            mp.setattr(tr, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg), orig_loss(lg, t))[1])
            loss = tr.train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev))
        torch.cuda.synchronize()
        trainable = fc.trainable((pattern, r))
        got = dict(loss=loss.cpu(), feat=seen['feat'].detach().cpu(), logits=seen['logits'].detach().permute(1, 0, 2).cpu(),
                   grads={k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None},
                   params={k: p.detach().cpu().clone() for k, p in net.named_parameters()},
                   running={k: b.detach().cpu().clone() for k, b in net.named_buffers() if 'running' in k},
                   nbt={k: int(b) for k, b in net.named_buffers() if 'num_batches' in k})
        assert list(got['grads']) == trainable, pattern
        bad = check_against_f64(got, w64, w32, c['B'], c['N']) + check_adam(sd, got, ADAM)
        assert not bad, pattern + '\n' + '\n'.join(str(b) for b in bad)
        for k in fc.param_names(r):
            assert torch.equal(got['params'][k], sd[k]) == (k not in trainable), (pattern, k)


def test_b3_flat_bucket_dp(dev, b3):
    """FlatBucketDP (world size 1) with the bf16x3 encoder: every gradient is born in the bucket and is, byte for byte, the
    gradient of the same step without the bucket."""
    from gnn_pathplanning_amd import training as tr
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    B, N = 8, 4
    sd, obs, S, tgt = make_case(B, N, seed=8403, margin=False)
    grads = []
    for bucket in (False, True):
        net = DecentralPlannerNet(CfgB3(N, 3, dev)).to(dev)
        net.load_state_dict(sd)
        net.train()
        dp = tr.FlatBucketDP(net) if bucket else None
        try:
            opt = tr.FusedAdam(net.parameters(), lr=ADAM[0], weight_decay=ADAM[1])
            tr.train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev), dp=dp)
            torch.cuda.synchronize()
            if bucket:
                for p, v in zip(dp.params, dp.views):
                    assert dp._in_bucket(p.grad, v)
            grads.append({k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()})
        finally:
            if dp is not None:
                dp.close()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k

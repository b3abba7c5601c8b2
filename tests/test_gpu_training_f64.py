"""GPU (-m gpu): the training step (BASELINE config 4) against a float64 statement of the same step.

The train-mode kernels (csrc/train_encoder.hip, csrc/train_ops.hip, the graph filter's training launches) are exact
fp32: fp32 MFMA and fmaf, fixed reduction orders.  Their error against float64 must therefore be of the size of any
other fp32 implementation's, and the yardstick is the same statement run by torch in fp32 on the CPU.  Per tensor
(`gap`): RMS error <= RMS_K x the fp32 RMS error and largest error <= MAX_K x the fp32 largest error, each + ULPS units
in the last place of the tensor's scale.  Two fp32 implementations that sum in different orders make independent
roundoff of the same size; over the few hundred to few hundred thousand entries of a tensor their RMS errors agree to
well under 2x and their maxima (a tail statistic) to under 4x, and the factors allow 2x on top.  The bugs this is for
sit far outside: the biased instead of the unbiased variance in the running statistics is a factor 1 + 1 / (m - 1)
(1.3e-4 at layer 0, B = 64), a weight-gradient split lost from a reduction is a few per cent of that gradient, and
one-pass BatchNorm statistics (s2 / m - mean^2) lose every digit once a channel's mean is 1e3 x its spread.

Outputs compared: loss, logits, encoder features, every parameter gradient, running mean / var,
num_batches_tracked, and the parameters after one FusedAdam step (against torch.optim.Adam in float64 on the same
gradients).  A conv bias in front of train-mode BatchNorm has an exactly-zero gradient: it is held to the same
yardstick with the ulps taken of the roundoff a sum of B x P terms of the layer's weight-gradient size makes.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as tF

from f64_yardstick import ULP, ULPS, gap
from oracle import policy_oracle as orc
from policy_f64_cases import filter_stack

pytestmark = pytest.mark.gpu

CONV = (0, 4, 7, 11, 14)
BN = (1, 5, 8, 12, 15)
POS = (121, 25, 25, 4, 4)                 # positions per image at each convolution's output
EPS, MOMENTUM = 1e-5, 0.1
KNOB_WGS, KNOB_FUSED = 17, 19


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from gnn_pathplanning_amd import _native
    _native.lib()
    return torch.device('cuda:0')


# ---- the float64 statement -----------------------------------------------------------------------------------------
def statement(sd, S, obs, tgt, N, dtype, frozen=None, relu=None):
    """One training step's forward and backward in `dtype` on the CPU, after the reference (agents/
    decentralplannerlocal.py:287-317 over graphs/models/decentralplanner.py:278-318): per-agent train-mode encoder calls
    (BatchNorm over that call's batch, N sequential running-statistics updates), compressMLP, the L graph-filter layers
    with their ReLUs (a GSO with more nodes than agents zero-pads the signal), the action head, the loss = mean over
    agents of CrossEntropy against the first arg-max of the target, every gradient by autograd.
    frozen(name): the parameters that take no gradient (requires_grad_(False) and nothing else: train-mode BatchNorm of a
    frozen encoder still uses batch statistics and updates the running ones) -- they are absent from 'grads'.
    relu(name, pre-activation), name = 'compress' | 'GFL.<2l>': as policy_f64_cases.filter_stack."""
    p = {k: v.to(dtype).clone().requires_grad_(not (frozen is not None and frozen(k))) for k, v in sd.items()
         if v.dtype.is_floating_point and 'running' not in k}
    run = {k: v.to(dtype).clone() for k, v in sd.items() if 'running' in k}
    nbt = {k: int(v) for k, v in sd.items() if 'num_batches' in k}
    B = obs.shape[0]
    x = obs.to(dtype)
    enc, comp = [], []
    for n in range(N):
        t = x[:, n]
        for li in range(5):
            t = tF.conv2d(t, p['ConvLayers.%d.weight' % CONV[li]], p['ConvLayers.%d.bias' % CONV[li]], padding=1)
            bn = 'ConvLayers.%d.' % BN[li]
            t = tF.batch_norm(t, run[bn + 'running_mean'], run[bn + 'running_var'], p[bn + 'weight'], p[bn + 'bias'],
                              training=True, momentum=MOMENTUM, eps=EPS)
            nbt[bn + 'num_batches_tracked'] += 1
            t = tF.relu(t)
            if orc.POOL_AFTER[li]:
                t = tF.max_pool2d(t, 2)
        enc.append(t.reshape(B, 128))
        pre = tF.linear(enc[-1], p['compressMLP.0.weight'], p['compressMLP.0.bias'])
        comp.append(tF.relu(pre) if relu is None else relu('compress', pre))
    h = torch.stack(comp, 2)                                             # [B,F,N]
    S4 = (S.unsqueeze(1) if S.dim() == 3 else S).to(dtype)               # [B,E,Ns,Ns]
    h = filter_stack(h, S4, p, N, relu)
    logits = torch.stack([tF.linear(h[:, :, n], p['actionsMLP.0.weight'], p['actionsMLP.0.bias'])
                          for n in range(N)], 1)                          # [B,N,5]
    labels = tgt.argmax(-1)                                              # first maximum
    loss = sum(tF.cross_entropy(logits[:, n], labels[:, n]) for n in range(N)) / N
    if loss.requires_grad:
        loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), feat=torch.stack(enc, 1).detach(),
                grads={k: v.grad for k, v in p.items() if v.requires_grad}, running=run, nbt=nbt)


def without_pool_near_ties(sd, obs, draw, tau=(1e-5, 0, 2e-6, 0, 2e-6), rounds=50):
    """obs with every sample that puts a near-tie into a 2x2 max-pool window (in the float64 forward) drawn again.
    The gradient is discontinuous where the two largest values of a window are equal: when they are within the
    roundoff of fp32 arithmetic, a correct fp32 kernel and float64 may route the window's gradient to different
    positions (an O(1) difference of that gradient entry; binary observations make such windows frequent at layer 0
    -- a few per thousand samples at 1e-6 relative).  With no window's two largest values closer than `tau` (of the
    window's largest value at layer 0, which sees the observations through one convolution; of the largest value of
    the (agent, channel) at the deeper pools), a different choice needs an activation error far beyond fp32
    roundoff."""
    obs = obs.clone()
    B, N = obs.shape[:2]
    for _ in range(rounds):
        bad = set()
        with torch.no_grad():
            for n in range(N):
                t = obs[:, n].double()
                for li in range(5):
                    t = tF.conv2d(t, sd['ConvLayers.%d.weight' % CONV[li]].double(),
                                  sd['ConvLayers.%d.bias' % CONV[li]].double(), padding=1)
                    bn = 'ConvLayers.%d.' % BN[li]
                    t = tF.relu(tF.batch_norm(t, None, None, sd[bn + 'weight'].double(), sd[bn + 'bias'].double(),
                                              training=True, eps=EPS))
                    if orc.POOL_AFTER[li]:
                        H = t.shape[-1] // 2 * 2
                        w = t[..., :H, :H].unfold(2, 2, 2).unfold(3, 2, 2)
                        top = w.reshape(*w.shape[:4], 4).topk(2, -1).values
                        # layer 0: relative to the window's own maximum (its near-ties stay put when other samples
                        # of the batch change); deeper layers: to the largest value of the (agent, channel)
                        scale = top[..., 0] if li == 0 else t.amax((0, 2, 3)).reshape(1, -1, 1, 1)
                        near = (top[..., 0] > 0) & (top[..., 0] - top[..., 1] > 0) & \
                            (top[..., 0] - top[..., 1] < tau[li] * scale)
                        bad.update((b, n) for b in near.flatten(1).any(1).nonzero().flatten().tolist())
                        t = tF.max_pool2d(t, 2)
        if not bad:
            return obs
        for b, n in sorted(bad):
            obs[b, n] = draw(*obs.shape[2:])
    raise AssertionError('could not draw observations without max-pool near-ties')


def centre_pre_activations(sd, S, obs, N):
    """Set the compress layer's and every graph filter's bias so that each output feature's pre-activation has its
    mean 3 standard deviations (over the batch's rows) above zero, layer by layer in the float64 forward."""
    with torch.no_grad():
        sdd = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}
        B = obs.shape[0]
        enc = []
        for n in range(N):
            t = obs[:, n].double()
            for li in range(5):
                t = tF.conv2d(t, sdd['ConvLayers.%d.weight' % CONV[li]], sdd['ConvLayers.%d.bias' % CONV[li]], padding=1)
                bn = 'ConvLayers.%d.' % BN[li]
                t = tF.relu(tF.batch_norm(t, None, None, sdd[bn + 'weight'], sdd[bn + 'bias'], training=True, eps=EPS))
                if orc.POOL_AFTER[li]:
                    t = tF.max_pool2d(t, 2)
            enc.append(t.reshape(B, 128))
        W, b = sdd['compressMLP.0.weight'], sdd['compressMLP.0.bias']
        pre = torch.stack(enc, 1) @ W.t()                                  # [B,N,F] without the bias
        shift = 3 * pre.std((0, 1)) - pre.mean((0, 1))
        sd['compressMLP.0.bias'] = shift.float()
        h = tF.relu(pre + shift).permute(0, 2, 1)                         # [B,F,N]
        S4 = (S.unsqueeze(1) if S.dim() == 3 else S).double()
        Ns, l = S4.shape[-1], 0
        while 'GFL.%d.weight' % (2 * l) in sd:
            w = sdd['GFL.%d.weight' % (2 * l)]
            z0 = torch.cat([h, h.new_zeros(B, h.shape[1], Ns - N)], 2) if Ns > N else h
            y = 0
            for e in range(w.shape[1]):
                z = z0
                for k in range(w.shape[2]):
                    if k:
                        z = z @ S4[:, e]
                    y = y + torch.einsum('fg,bgn->bfn', w[:, e, k], z)
            y = y[:, :, :N]
            shift = 3 * y.std((0, 2)) - y.mean((0, 2))                    # per output feature
            sd['GFL.%d.bias' % (2 * l)] = shift.reshape(-1, 1).float()
            h = tF.relu(y + shift.reshape(1, -1, 1))
            l += 1


# ---- the planner under test ----------------------------------------------------------------------------------------
class Cfg:
    """K: taps of every layer, or a list of L values; widths: output features per layer (default: 128 each)."""

    def __init__(self, N, K, dev, L=1, E=1, widths=None):
        self.num_agents, self.device = N, dev
        if isinstance(K, (list, tuple)):
            assert len(K) == L
            self.nGraphFilterTaps = list(K)
        else:
            self.nGraphFilterTaps = [K] * L if L > 1 else K
        if widths is not None:
            assert len(widths) == L
            self.dimNodeSignals = list(widths)
        elif L > 1:
            self.dimNodeSignals = [128] * L
        self.numEdgeFeatures = E


def make_case(B, N, K=3, L=1, E=1, Ns=None, seed=0, edge=None, fp64_gso=False, real_obs=False, tie=False,
              margin=None, widths=None):
    """Parameters (the planner's own init + non-trivial BatchNorm state), observations, GSO and targets.

    margin (default: from 640 agent-samples on): keep the step's decisions away from their discontinuities.  A ReLU
    whose input is within roundoff of zero, like a max-pool near-tie, lets a correct fp32 kernel route one gradient
    entry differently from float64 -- an O(1) change of that entry that spreads through every gradient below it.
    The chance of at least one such value grows with the batch (in the initialised regime it is already sizeable at
    64 x 10).  So the larger batches, which are here for the kernels' tiling switch points, run with the BatchNorm
    shifts + 3 and the compress / graph-filter biases centring each pre-activation 3 standard deviations above zero
    (set from the float64 forward); the small ones run in the plain regime."""
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in DecentralPlannerNet(Cfg(N, K, 'cpu', L, E, widths)).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for li in range(5):
        bn = 'ConvLayers.%d.' % BN[li]
        C = sd[bn + 'weight'].shape[0]
        sd[bn + 'weight'] = 1.0 + 0.1 * torch.randn(C, generator=g)
        sd[bn + 'bias'] = 0.1 * torch.randn(C, generator=g)
        sd[bn + 'running_mean'] = 0.1 * torch.randn(C, generator=g)
        sd[bn + 'running_var'] = 0.5 + torch.rand(C, generator=g)
    margin = B * N >= 640 if margin is None else margin
    if margin:
        for li in range(5):
            sd['ConvLayers.%d.bias' % BN[li]] += 3.0
    for e in (edge or '').split(','):
        if e.startswith('bias0+'):              # pre-BN offsets: cancel exactly in train-mode BatchNorm
            sd['ConvLayers.0.bias'] += float(e[6:])
        elif e.startswith('bias2+'):
            sd['ConvLayers.7.bias'] += float(e[6:])
        elif e == 'zero_var':                   # a channel of zero variance: output beta, zero gamma gradient
            for li, c in ((0, 5), (2, 9), (4, 17)):
                sd['ConvLayers.%d.weight' % CONV[li]][c] = 0.0
        elif e == 'gamma':                      # gamma = 0, negative gamma, a channel dead after ReLU (beta = -10)
            for li in range(5):
                w = sd['ConvLayers.%d.weight' % BN[li]]
                w[0] = 0.0
                w[1::3] *= -1.0
                sd['ConvLayers.%d.bias' % BN[li]][2] = -10.0
        elif e == 'head1e3':                    # large logits into the loss
            sd['actionsMLP.0.weight'] *= 1e3
    Ns = Ns or N
    draw = (lambda *shape: torch.randn(*shape, generator=g)) if real_obs else \
        (lambda *shape: (torch.rand(*shape, generator=g) < 0.25).float())
    obs = without_pool_near_ties(sd, draw(B, N, 3, 11, 11), draw)
    S = torch.from_numpy(orc.synth_gso_geometric(B * E, Ns, max(8, 2 * Ns), seed=seed + 2))
    S = S.reshape(B, E, Ns, Ns) if E > 1 else S
    S = S if fp64_gso else S.float()
    if margin:
        centre_pre_activations(sd, S, obs, N)
    if tie:                                     # targets with several ones: the first maximum is the label
        tgt = (torch.rand(B, N, 5, generator=g) < 0.5).float()
        tgt[..., 0] = 0.0
    else:
        tgt = tF.one_hot(torch.randint(0, 5, (B, N), generator=g), 5).float()
    return sd, obs, S, tgt


def run_planner(dev, sd, obs, S, tgt, N, K, L, E, via_step, monkeypatch, adam=None, widths=None):
    """The HIP training step: forward (encoder features captured at the autograd Function), loss, backward --
    through training.train_step() (fused loss launch, deferred parameter-gradient products, one FusedAdam step) or
    through policy_loss(...).backward()."""
    from gnn_pathplanning_amd import decentralplanner as dp
    from gnn_pathplanning_amd import training
    seen = {}
    orig, orig_loss = dp._EncoderTrainFunction.apply, training._policy_loss_and_grad
    with monkeypatch.context() as mp:
        mp.setattr(dp._EncoderTrainFunction, 'apply', lambda *a: seen.setdefault('feat', orig(*a)))
        # train_step's fused loss launch: the logits [N,B,5] it is handed
        mp.setattr(training, '_policy_loss_and_grad', lambda lg, t: (seen.setdefault('logits', lg), orig_loss(lg, t))[1])
        res = _step(dev, dp, sd, obs, S, tgt, N, K, L, E, via_step, adam, widths)
    res['feat'] = seen['feat'].detach().cpu()
    if via_step:
        res['logits'] = seen['logits'].detach().permute(1, 0, 2).cpu()
    return res


def _step(dev, dp, sd, obs, S, tgt, N, K, L, E, via_step, adam, widths=None):
    from gnn_pathplanning_amd.training import FusedAdam, policy_loss, train_step
    net = dp.DecentralPlannerNet(Cfg(N, K, dev, L, E, widths)).to(dev)
    net.load_state_dict(sd)
    net.train()
    res = {}
    if via_step:
        lr, wd, state = adam
        opt = FusedAdam(net.parameters(), lr=lr, weight_decay=wd)
        if state is not None:
            opt.load_state_dict(state(net, opt))
        loss = train_step(net, opt, obs.to(dev), tgt.to(dev), S.to(dev))
        res['params'] = {k: p.detach().cpu().clone() for k, p in net.named_parameters()}
    else:
        net.addGSO(S.to(dev))
        out = net(obs.to(dev))
        loss = policy_loss(out, tgt.to(dev))
        loss.backward()
        res['logits'] = torch.stack(list(out), 1).detach().cpu()
    torch.cuda.synchronize()
    res['loss'] = loss.detach().cpu()
    res['grads'] = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    res['running'] = {k: b.detach().cpu().clone() for k, b in net.named_buffers() if 'running' in k}
    res['nbt'] = {k: int(b) for k, b in net.named_buffers() if 'num_batches' in k}
    return res


def grad_scale(k, g64, B, N):
    """The scale the yardstick's floor is taken of for the gradient of parameter k (None: the gradient's own largest
    entry); g64: the float64 gradients by name."""
    li = CONV.index(int(k.split('.')[1])) if k.startswith('ConvLayers.') and int(k.split('.')[1]) in CONV else None
    if li is not None and k.endswith('.bias'):
        return g64['ConvLayers.%d.weight' % CONV[li]].abs().max().item() * np.sqrt(B * POS[li])
    if k.endswith('.bias') and not k.startswith('ConvLayers.'):
        # a sum over all N x B rows of terms that nearly cancel (softmax - one-hot): its roundoff grows with the
        # square root of the row count, in units of the result's own scale
        return g64[k].abs().max().item() * np.sqrt(B * N)
    return None


def check_against_f64(got, w64, w32, B, N):
    bad = []

    def cmp(name, a, b64, b32, scale=None):
        ok, rep = gap(a, b64, b32, scale)
        if not ok:
            bad.append((name, rep))
    cmp('logits', got['logits'], w64['logits'], w32['logits'])
    # the loss is ONE number, and the ratio of two single roundoff samples says little: besides the yardstick it may
    # carry what its inputs carry -- a mean of cross entropies moves by at most 2 max |d logit|
    ok, rep = gap(got['loss'], w64['loss'], w32['loss'])
    dlog = (got['logits'].double() - w64['logits']).abs().max().item()
    if not ok and rep['max'] > 2 * dlog + ULPS * ULP * rep['scale']:
        bad.append(('loss', rep, 'max |d logit| %.3g' % dlog))
    cmp('feat', got['feat'], w64['feat'], w32['feat'])
    for k, g in got['grads'].items():
        cmp(k, g, w64['grads'][k], w32['grads'][k], grad_scale(k, w64['grads'], B, N))
    for k, r in got['running'].items():
        cmp(k, r, w64['running'][k], w32['running'][k])
    for k, c in got['nbt'].items():
        if c != w64['nbt'][k]:
            bad.append((k, c, w64['nbt'][k]))
    return bad


def one_case(dev, monkeypatch, B, N, K=3, L=1, E=1, Ns=None, seed=0, edge=None, fp64_gso=False, real_obs=False,
             tie=False, via_step=True, adam=(1e-3, 1e-5, None), widths=None):
    sd, obs, S, tgt = make_case(B, N, K, L, E, Ns, seed, edge, fp64_gso, real_obs, tie, widths=widths)
    w64 = statement(sd, S, obs, tgt, N, torch.float64)
    w32 = statement(sd, S, obs, tgt, N, torch.float32)
    got = run_planner(dev, sd, obs, S, tgt, N, K, L, E, via_step, monkeypatch, adam if via_step else None, widths)
    # every parameter's gradient is compared -- those below the filter stack (GFL.0, compressMLP, the encoder) are the
    # ones that change when a cotangent on the extra nodes of a larger GSO is carried from layer to layer
    assert set(got['grads']) == set(w64['grads']) == set(w32['grads'])
    assert {'compressMLP.0.weight', 'compressMLP.0.bias', 'actionsMLP.0.weight'} <= set(got['grads'])
    assert {'GFL.%d.%s' % (2 * l, n) for l in range(L) for n in ('weight', 'bias')} <= set(got['grads'])
    bad = check_against_f64(got, w64, w32, B, N)
    if via_step:
        bad += check_adam(sd, got, adam)
    assert not bad, '\n'.join(str(b) for b in bad)
    return got, w64, w32


def check_adam(sd, got, adam):
    """FusedAdam's step against torch.optim.Adam in float64 (yardstick: the same in fp32) on the kernel's gradients.
    The hyperparameters are those the kernel is handed: gnnpp_adam_step takes lr, betas, eps and weight decay as fp32
    (1 - 0.9f differs from 0.1 by 2.4e-7 relative, which a state far from the current gradient turns into ~1e-4 of a
    step)."""
    lr, wd, state = adam
    f32 = lambda v: float(np.float32(v))                   # noqa: E731
    names = list(got['grads'])
    res = {}
    for dt in (torch.float64, torch.float32):
        ps = [sd[k].to(dt).clone().requires_grad_(True) for k in names]
        opt = torch.optim.Adam(ps, lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(wd))
        if state is not None:
            for k, p in zip(names, ps):
                st = state.torch_state[k]
                opt.state[p] = {'step': torch.tensor(float(st['step']), dtype=torch.float32),
                                'exp_avg': st['exp_avg'].to(dt).clone(), 'exp_avg_sq': st['exp_avg_sq'].to(dt).clone()}
        for k, p in zip(names, ps):
            p.grad = got['grads'][k].to(dt)
        opt.step()
        res[dt] = {k: p.detach() for k, p in zip(names, ps)}
    bad = []
    for k in names:
        ok, rep = gap(got['params'][k], res[torch.float64][k], res[torch.float32][k])
        if not ok:
            bad.append(('adam ' + k, rep))
    return bad


# ---- shapes on the kernels' switch points ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,N', [(1, 1), (1, 10), (2, 3), (7, 3), (64, 10), (128, 10), (129, 10), (410, 10), (5, 17),
                                 (33, 50), (2, 120)])
def test_training_step_against_float64(dev, monkeypatch, B, N):
    """Through train_step(): 1 x 1 .. 7 x 3 (ragged image tiles), 64 x 10 (config 4's shard), 128 / 129 x 10 (the
    weight-gradient heuristic switches at 1 280 agent-samples), 410 x 10 (above the 4 096-row fork threshold), 5 x 17,
    33 x 50, N = 120 (the graph filter's dense path beyond 112 rows)."""
    one_case(dev, monkeypatch, B, N, seed=B * 1000 + N)
    if (B, N) == (64, 10):                                   # and the logits, through policy_loss(...).backward()
        one_case(dev, monkeypatch, B, N, seed=B * 1000 + N, via_step=False)


@pytest.mark.parametrize('B,N,K,L,E,Ns,fp64_gso', [(5, 6, 3, 1, 1, 9, False), (6, 7, 1, 1, 1, None, False),
                                                   (6, 7, 4, 1, 1, None, True), (4, 5, 2, 1, 2, None, False),
                                                   (4, 5, 3, 2, 1, None, False), (3, 4, 2, 2, 2, None, True),
                                                   (4, 5, 3, 2, 1, 8, False), (3, 4, 2, 2, 2, 7, True),
                                                   (3, 5, 2, 3, 1, 8, False), (2, 100, 2, 2, 1, 120, False)])
def test_planner_variants_against_float64(dev, monkeypatch, B, N, K, L, E, Ns, fp64_gso):
    """A GSO with more nodes than agents, K = 1 and 4, E = 2 edge features, two filter layers (the multilayer path
    without the step's packed filter), an fp64 GSO; through plain policy_loss(...).backward() as well.  Several layers
    AND a larger GSO (L = 2, L = 2 with E = 2 and an fp64 GSO, L = 3, and 100 agents on 120 nodes: the dense training
    form): every layer zero-pads its input again (graphML.py:2464-2476), so neither an activation nor a cotangent on
    the extra nodes passes from one layer to the next -- the statement (filter_stack) re-pads per layer."""
    one_case(dev, monkeypatch, B, N, K, L, E, Ns, seed=B + 10 * N + 100 * K, fp64_gso=fp64_gso)
    one_case(dev, monkeypatch, B, N, K, L, E, Ns, seed=B + 10 * N + 100 * K, fp64_gso=fp64_gso, via_step=False)


def test_planner_unequal_widths_larger_gso_against_float64(dev, monkeypatch):
    """Two layers of unequal widths (128 -> 64 -> 48) and taps (2, 3), E = 2, on a GSO of 9 nodes for 6 agents."""
    kw = dict(K=[2, 3], L=2, E=2, Ns=9, seed=4242, widths=[64, 48])
    one_case(dev, monkeypatch, 4, 6, **kw)
    one_case(dev, monkeypatch, 4, 6, via_step=False, **kw)


@pytest.mark.parametrize('knob,value', [(KNOB_WGS, 16), (KNOB_WGS, 2048), (KNOB_FUSED, 0)])
def test_training_knobs_against_float64(dev, monkeypatch, knob, value):
    """Every training knob setting against float64 itself, not only against the default setting (the defaults, 128 / 256
    weight-gradient workgroups by batch and fused running statistics, are the other tests)."""
    from gnn_pathplanning_amd import _native
    Lb = _native.lib()
    old = Lb.gnnpp_get_tuning(knob)
    assert Lb.gnnpp_set_tuning(knob, value) == 0
    try:
        for B, N in ((64, 10), (7, 3)):
            one_case(dev, monkeypatch, B, N, seed=knob * 100 + B)
    finally:
        assert Lb.gnnpp_set_tuning(knob, old) == 0


# ---- value edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('edge,B,N,kw', [('bias0+10', 64, 10, {}), ('bias0+100', 64, 10, {}),
                                         ('bias0+1000', 64, 10, {}), ('bias0+1000', 7, 3, {}),
                                         ('bias2+100', 16, 5, {}), ('zero_var', 16, 5, {}), ('gamma', 16, 5, {}),
                                         (None, 16, 5, {'real_obs': True}), ('head1e3', 16, 5, {'tie': True}),
                                         ('bias0+100,gamma', 9, 4, {'via_step': False})])
def test_value_edges_against_float64(dev, monkeypatch, edge, B, N, kw):
    """Pre-BatchNorm offsets (conv-0 bias + 10 / 100 / 1000, conv-2 bias + 100: exact cancellations the one-pass
    statistics s2 / m - mean^2 lost), a zero-variance channel (zero conv weights: output = beta, d gamma = 0), gamma = 0
    and negative, a channel dead after ReLU, real-valued observations, head weights x 1e3 with tied targets."""
    got, _, _ = one_case(dev, monkeypatch, B, N, seed=7, edge=edge, **kw)
    if edge == 'zero_var':
        for li, c in ((0, 5), (2, 9), (4, 17)):
            assert got['grads']['ConvLayers.%d.weight' % BN[li]][c].item() == 0.0


class _AdamState:
    """An optimizer state near step `t`: moments of the size a long run leaves, for FusedAdam and for torch."""

    def __init__(self, t, seed):
        self.t, self.seed, self.torch_state = t, seed, {}

    def __call__(self, net, opt):
        g = torch.Generator().manual_seed(self.seed)
        sd = opt.state_dict()
        for i, (k, p) in enumerate(net.named_parameters()):
            m = 1e-3 * torch.randn(p.shape, generator=g)
            v = 1e-6 * torch.rand(p.shape, generator=g)
            self.torch_state[k] = {'step': self.t, 'exp_avg': m, 'exp_avg_sq': v}
            sd['state'][i] = {'exp_avg': m.to(p.device), 'exp_avg_sq': v.to(p.device)}
        # the device-side step counter: [steps, ...] (training.FusedAdam keeps the rest derived from it)
        ctr = torch.zeros(8, dtype=torch.float32)
        ctr[0] = float(self.t)
        sd['state']['gnnpp_group_0'] = {'counter': ctr.to(next(net.parameters()).device)}
        return sd


@pytest.mark.parametrize('t', [None, 9999])
def test_fused_adam_step_against_float64(dev, monkeypatch, t):
    """FusedAdam at step 1 and after loading a state near step 1e4, with weight decay, against torch.optim.Adam in
    float64 on the same gradients."""
    one_case(dev, monkeypatch, 16, 5, seed=3, adam=(1e-3, 1e-4, _AdamState(t, 11) if t else None))


# ---- BatchNorm settings the kernels do not compute ---------------------------------------------------------------------
@pytest.mark.parametrize('setting', ['eps', 'momentum', 'momentum_none', 'track_some', 'uniform'])
@pytest.mark.parametrize('training', [True, False])
def test_batchnorm_settings_match_torch_or_raise(dev, setting, training):
    """The kernels take one eps and one momentum for all five BatchNorm2d layers: a planner with per-layer values,
    momentum=None (torch's cumulative average) or running statistics tracked by some layers only either matches the
    same nn.Module on torch (CPU, float64) or raises GnnppError -- never a silent difference."""
    from gnn_pathplanning_amd import _native
    from gnn_pathplanning_amd.decentralplanner import DecentralPlannerNet
    B, N = 4, 3
    sd, obs, S, tgt = make_case(B, N, seed=21)

    def planner(device):
        net = DecentralPlannerNet(Cfg(N, 3, device)).to(device)
        net.load_state_dict(sd)
        for i, bi in enumerate(BN):
            bn = net.ConvLayers[bi]
            if setting == 'eps':
                bn.eps = 1e-5 * (1 + i)
            elif setting == 'momentum':
                bn.momentum = 0.1 + 0.05 * i
            elif setting == 'momentum_none':
                bn.momentum = None
            elif setting == 'track_some' and i == 2:
                bn.track_running_stats = False
                bn.running_mean = bn.running_var = bn.num_batches_tracked = None
        return net
    net, ref = planner(dev), planner('cpu').double()
    net.train(training)
    ref.train(training)
    net.addGSO(S.to(dev))
    try:
        out = net(obs.to(dev))
    except _native.GnnppError:
        assert setting != 'uniform'
        return
    torch.cuda.synchronize()
    with torch.no_grad():
        t = obs.double()
        enc = []
        for n in range(N):                                 # the module's own layers, per agent call
            x = t[:, n]
            for m in ref.ConvLayers:
                x = m(x)
            enc.append(torch.relu(ref.compressMLP[0](x.reshape(B, 128))))
        h = torch.stack(enc, 2)
        S4 = S.double().unsqueeze(1)
        w, b = ref.GFL[0].weight, ref.GFL[0].bias
        y = 0
        for k in range(w.shape[2]):
            z = h if k == 0 else z @ S4[:, 0]
            y = y + torch.einsum('fg,bgn->bfn', w[:, 0, k], z)
        h = torch.relu(y + b)
        want = torch.stack([ref.actionsMLP[0](h[:, :, n]) for n in range(N)], 1)
    got = torch.stack(list(out), 1).detach().cpu().double()
    assert (got - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item()), setting
    for (k, a), (_, r) in zip(net.named_buffers(), ref.named_buffers()):
        if a is not None and r is not None and a.dtype.is_floating_point:
            assert (a.cpu().double() - r).abs().max().item() <= 1e-5, (setting, k)
        elif a is not None and r is not None:
            assert int(a) == int(r), (setting, k)

"""Neighbour lists as the hand-over between the rollout simulator and the team filter: the shared instances and runners
of tests/test_emu_rollout_lists.py, tests/test_emu_filter_team_lists.py (host emulation) and
tests/test_gpu_rollout_lists.py, tests/test_gpu_filter_team_lists.py, tests/test_gpu_rollout_lists_loop.py (MI355X).
A plain helper module, not a conftest.

Every comparison is an equality.  Two references, both independent of the code under test:
  * lists from positions: the dense S, radius and connected of oracle.rollout_oracle.communication_gso, turned per
    column into the ascending non-zero rows and their float32 weights; and gnnpp_team_lists_from_dense of
    gnnpp_rollout_gso's S (the existing kernels);
  * the filter on lists: the existing dense-S team calls on the same S.
A block is handed over filled with 0xFF bytes (count -1, index 65535, weight NaN): whatever is read must have been
written by the call."""
import ctypes

import numpy as np

import filter_f64_cases as fc
import filter_team_cases as tc
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED


# ---- the block ---------------------------------------------------------------------------------------------------
def layout(graphs, N):
    """(offset of cnt, of idx, of val, total bytes, Np) of a lists block, restated from include/gnnpp.h."""
    Np = (N + 3) & ~3
    up = lambda v: (v + 15) & ~15                                              # noqa: E731
    idx = up(graphs * N * 4)
    val = idx + up(graphs * N * Np * 2)
    return 0, idx, val, val + up(graphs * N * Np * 4), Np


def views(block, graphs, N):
    """cnt [graphs,N] int32, idx [graphs,N,Np] uint16, val [graphs,N,Np] float32 views of a uint8 numpy block."""
    c, i, v, total, Np = layout(graphs, N)
    assert block.dtype == np.uint8 and block.size >= total
    return (block[c:c + graphs * N * 4].view(np.int32).reshape(graphs, N),
            block[i:i + graphs * N * Np * 2].view(np.uint16).reshape(graphs, N, Np),
            block[v:v + graphs * N * Np * 4].view(np.float32).reshape(graphs, N, Np))


def fresh_block(bk, graphs, N):
    nbytes = bk.lib.gnnpp_team_lists_bytes(graphs, N)
    assert nbytes == layout(graphs, N)[3] and nbytes % 16 == 0
    return bk.put(np.full(nbytes, 0xFF, np.uint8)), nbytes


def lists_of_dense(S32):
    """Per graph and column: (ascending non-zero rows, their float32 weights) of S32 [graphs,N,N]."""
    out = []
    for g in range(S32.shape[0]):
        cols = []
        for n in range(S32.shape[1]):
            rows = np.nonzero(S32[g, :, n])[0]
            cols.append((rows, S32[g, rows, n]))
        out.append(cols)
    return out


def check_block(name, block, want):
    """cnt, the entries and the padding up to the next multiple of four of every column, bit for bit."""
    graphs, N = len(want), len(want[0])
    cnt, idx, val = views(block, graphs, N)
    for g in range(graphs):
        for n in range(N):
            rows, w = want[g][n]
            k = len(rows)
            assert cnt[g, n] == k, (name, g, n, int(cnt[g, n]), k)
            k4 = (k + 3) & ~3
            assert (idx[g, n, :k] == rows).all() and (idx[g, n, k:k4] == 0).all(), (name, g, n)
            assert val[g, n, :k].tobytes() == w.astype(np.float32).tobytes(), (name, g, n)
            assert val[g, n, k:k4].tobytes() == bytes(4 * (k4 - k)), (name, g, n)


def same_lists(name, a, b, graphs, N):
    """Two blocks agree over cnt and the first roundup4(cnt) entries of every column."""
    ca, ia, va = views(a, graphs, N)
    cb, ib, vb = views(b, graphs, N)
    assert (ca == cb).all(), name
    live = np.arange(ia.shape[2])[None, None, :] < ((ca + 3) & ~3)[:, :, None]
    assert (ia[live] == ib[live]).all(), name
    assert va[live].tobytes() == vb[live].tobytes(), name


# ---- instances: positions [B,N,2], initial radius [B], grow ------------------------------------------------------------
def _scatter(seed, B, N, W):
    g = np.random.default_rng(seed)
    return np.stack([np.stack(np.unravel_index(g.choice(W * W, N, replace=False), (W, W)), 1) for _ in range(B)])


def _chain(N, gap):
    return np.stack([np.zeros(N, np.int64), gap * np.arange(N)], 1)[None]


def _outlier():
    pos = _scatter(3, 1, 40, 8)
    pos[0, 17] = (60, 60)
    return pos


def _two_components():
    a, b = _scatter(4, 1, 35, 7), _scatter(5, 1, 31, 7)
    pos = np.concatenate([a, b + 40], 1)
    return pos[:, np.random.default_rng(6).permutation(66)]                     # (components interleaved by index)


def _packed_box():
    cells = np.stack(np.unravel_index(np.arange(132), (12, 11)), 1)[None]
    return cells[:, np.random.default_rng(7).permutation(132)[:130]]


CASES = [
    dict(name='N1', pos=_scatter(11, 2, 1, 6), radius=6.0, grow=1),
    dict(name='N2', pos=_scatter(12, 2, 2, 9), radius=2.0, grow=1),
    dict(name='N5', pos=_scatter(13, 2, 5, 9), radius=3.0, grow=1),
    dict(name='N5/nogrow', pos=_scatter(13, 2, 5, 9), radius=5.0, grow=0),
    dict(name='N17', pos=_scatter(14, 2, 17, 12), radius=3.0, grow=1),
    dict(name='N65', pos=_scatter(15, 1, 65, 24), radius=4.0, grow=1),
    dict(name='N130', pos=_scatter(16, 2, 130, 30), radius=5.0, grow=1),
    dict(name='N130/nogrow', pos=_scatter(16, 2, 130, 30), radius=4.5, grow=0),
    dict(name='N257', pos=_scatter(17, 1, 257, 40), radius=4.0, grow=1),
    dict(name='B3/radius_per_episode', pos=_scatter(18, 3, 70, 22), radius=[2.0, 5.5, 9.25], grow=0),
    dict(name='B3/radius_per_episode/grow', pos=_scatter(18, 3, 70, 22), radius=[1.5, 5.5, 30.0], grow=1),
    dict(name='outlier/nogrow', pos=_outlier(), radius=4.0, grow=0, connected=[0], empty_column=17),
    dict(name='two_components/nogrow', pos=_two_components(), radius=6.0, grow=0, connected=[0]),
    dict(name='sparse/grow', pos=_scatter(19, 2, 66, 60), radius=1.2, grow=1, min_growth=8),
    dict(name='packed_box/degree129', pos=_packed_box(), radius=20.0, grow=0, connected=[1], degree=129),
    dict(name='chain70', pos=_chain(70, 3), radius=3.5, grow=0, connected=[1]),
    dict(name='chain70/grow', pos=_chain(70, 3), radius=1.0, grow=1, connected=[1]),
    # the thread-per-agent kernels (N > 128, here past the 192 / 193 wave boundary) growing from a radius below 2, where
    # consecutive radii share an integer threshold (1.0, 1.1 .. 1.331 all admit d2 <= 1 only): rollout_team_lists_kernel
    # keeps its lists over such a trip, rollout_team_gso_kernel searches again; both must end at the oracle's radius
    dict(name='chain193/grow_from_1', pos=_chain(193, 3), radius=1.0, grow=1, connected=[1], min_growth=12),
]
GPU_CASES = [
    dict(name='B2N1024/map64/grow', pos=_scatter(20, 2, 1024, 64), radius=2.0, grow=1),
    dict(name='B2N1024/map64/nogrow', pos=_scatter(21, 2, 1024, 64), radius=6.0, grow=0),
]

_oracle_cache = {}


def oracle_lists(c):
    """(lists, radius [B], connected [B]) of the oracle for case c; computed once and shared."""
    if c['name'] not in _oracle_cache:
        from oracle import rollout_oracle as ro
        B = c['pos'].shape[0]
        r0 = np.broadcast_to(np.asarray(c['radius'], np.float64), (B,))
        out = [ro.communication_gso(c['pos'][b], float(r0[b]), bool(c['grow'])) for b in range(B)]
        S32 = np.stack([o[0] for o in out]).astype(np.float32)
        _oracle_cache[c['name']] = (lists_of_dense(S32), np.array([o[1] for o in out], np.float64),
                                    np.array([int(o[2]) for o in out], np.int32))
    return _oracle_cache[c['name']]


class State:
    """pos / radius / connected (/ S) of B episodes on a backend, and the gnnpp_rollout struct pointing at them."""

    def __init__(self, bk, c, with_S):
        from gnn_pathplanning_amd._native import RolloutStruct
        B, N = c['pos'].shape[:2]
        self.pos = bk.put(np.ascontiguousarray(c['pos'], np.int32))
        self.radius = bk.put(np.ascontiguousarray(np.broadcast_to(np.asarray(c['radius'], np.float64), (B,))))
        self.conn = bk.put(np.full(B, -7, np.int32))
        self.S = bk.put(np.full((B, N, N), np.nan, np.float32)) if with_S else None
        r = RolloutStruct()
        r.pos, r.B, r.N, r.radius, r.connected = self.pos.ptr.value, B, N, self.radius.ptr.value, self.conn.ptr.value
        r.S = self.S.ptr.value if with_S else None
        r.grow = int(c['grow'])
        self.r = r


def run_lists_case(bk, c):
    """gnnpp_rollout_lists of case c against the oracle's lists and against gnnpp_team_lists_from_dense of
    gnnpp_rollout_gso's S; radius and connected against both; a second call gives the same bytes."""
    B, N = c['pos'].shape[:2]
    want, want_r, want_c = oracle_lists(c)
    blocks = []
    for _ in range(2):
        st = State(bk, c, with_S=False)
        blk, nbytes = fresh_block(bk, B, N)
        assert bk.lib.gnnpp_rollout_lists(ctypes.byref(st.r), blk.ptr, nbytes, bk.stream) == 0, c['name']
        bk.sync()
        blocks.append(blk.get())
        radius, conn = st.radius.get(), st.conn.get()
    assert blocks[0].tobytes() == blocks[1].tobytes(), c['name']
    check_block(c['name'], blocks[0], want)
    assert radius.tobytes() == want_r.tobytes(), (c['name'], radius, want_r)
    assert (conn == want_c).all(), (c['name'], conn, want_c)
    # the existing kernels on the same state
    st = State(bk, c, with_S=True)
    assert bk.lib.gnnpp_rollout_gso(ctypes.byref(st.r), bk.stream) == 0
    blk, nbytes = fresh_block(bk, B, N)
    assert bk.lib.gnnpp_team_lists_from_dense(st.S.ptr, blk.ptr, nbytes, B, N, 0, bk.stream) == 0
    bk.sync()
    same_lists(c['name'], blocks[0], blk.get(), B, N)
    assert st.radius.get().tobytes() == radius.tobytes() and (st.conn.get() == conn).all(), c['name']
    # what the case is there for
    cnt = views(blocks[0], B, N)[0]
    if 'connected' in c:
        assert list(conn) == c['connected'], c['name']
    if 'empty_column' in c:
        assert cnt[0, c['empty_column']] == 0 and (np.delete(cnt[0], c['empty_column']) > 0).all()
    if 'degree' in c:
        assert (cnt == c['degree']).all() and layout(B, N)[4] == c['degree'] + 3
    if 'min_growth' in c:
        r0 = np.broadcast_to(np.asarray(c['radius'], np.float64), (B,))
        assert (radius > r0 * 1.1 ** (c['min_growth'] - 1)).all(), (c['name'], radius)
    return cnt


def run_lists_errors(bk):
    """gnnpp_team_lists_bytes / _from_dense / gnnpp_rollout_lists: the codes, and the block untouched on error."""
    lib = bk.lib
    assert lib.gnnpp_team_lists_bytes(0, 10) == 0 and lib.gnnpp_team_lists_bytes(2, 0) == 0
    assert lib.gnnpp_team_lists_bytes(2, 1025) == 0 and lib.gnnpp_team_lists_bytes(-1, 5) == 0
    for graphs, N in ((1, 1), (3, 5), (2, 130), (8, 1024)):
        assert lib.gnnpp_team_lists_bytes(graphs, N) == layout(graphs, N)[3]
        assert lib.gnnpp_team_lists_bytes(graphs, N) <= lib.gnnpp_lsigf_team_workspace_bytes(graphs, N, 128, 2, 1, 1)
    c = CASES[4]                                                               # N = 17
    B, N = c['pos'].shape[:2]
    need = lib.gnnpp_team_lists_bytes(B, N)
    S = bk.put(np.zeros((B, N, N), np.float32))

    def rollout(blk, nbytes, off=0, **kw):
        st = State(bk, c, with_S=False)
        for k, v in kw.items():
            setattr(st.r, k, v)
        ptr = ctypes.c_void_p(blk.ptr.value + off) if blk is not None else None
        rc = lib.gnnpp_rollout_lists(ctypes.byref(st.r), ptr, nbytes, bk.stream)
        bk.sync()
        assert st.conn.get()[0] == -7 or rc == 0
        return rc

    def dense(blk, nbytes, off=0, S=S, graphs=B, N=N):
        ptr = ctypes.c_void_p(blk.ptr.value + off) if blk is not None else None
        return lib.gnnpp_team_lists_from_dense(S.ptr if S is not None else None, ptr, nbytes, graphs, N, 0, bk.stream)

    table = (('short block', lambda b: rollout(b, need - 1)), ('misaligned block', lambda b: rollout(b, need, off=4)),
             ('NULL block', lambda b: rollout(None, need)), ('NULL pos', lambda b: rollout(b, need, pos=None)),
             ('NULL radius', lambda b: rollout(b, need, radius=None)), ('N = 0', lambda b: rollout(b, need, N=0)),
             ('N = 1025', lambda b: rollout(b, 1 << 30, N=1025)), ('B = 0', lambda b: rollout(b, need, B=0)),
             ('dense: short block', lambda b: dense(b, need - 1)), ('dense: misaligned', lambda b: dense(b, need, off=8)),
             ('dense: NULL block', lambda b: dense(None, need)), ('dense: NULL S', lambda b: dense(b, need, S=None)),
             ('dense: graphs = 0', lambda b: dense(b, need, graphs=0)), ('dense: N = 1025', lambda b: dense(b, 1 << 30, N=1025)))
    for name, call in table:
        blk = bk.put(np.full(need + 16, 0xFF, np.uint8))
        assert call(blk) == ERR_ARG, name
        bk.sync()
        assert (blk.get() == 0xFF).all(), name
    # ... and both calls work with exactly the bytes they ask for
    blk = bk.put(np.full(need, 0xFF, np.uint8))
    assert rollout(blk, need) == 0 and dense(blk, need) == 0
    bk.sync()
    assert (views(blk.get(), B, N)[0] == 0).all()                              # (S = 0: no neighbours)


# ---- the filter on lists against the dense-S team calls ---------------------------------------------------------------
def _s_variant(c, S):
    S = tc.shape_s(S, c.get('s'), c['seed'])
    return S.astype(np.float64) if c.get('f64') else S


def filter_lists(bk, S, N):
    """gnnpp_team_lists_from_dense of S [.., N, N] (numpy, fp32 or fp64) in a fresh block."""
    graphs = S.size // (N * N)
    blk, nbytes = fresh_block(bk, graphs, N)
    Sd = bk.put(S)
    assert bk.lib.gnnpp_team_lists_from_dense(Sd.ptr, blk.ptr, nbytes, graphs, N, int(S.dtype == np.float64),
                                              bk.stream) == 0
    bk.sync()
    return blk


def run_filter_equal(bk, c, prec):
    """gnnpp_lsigf_team_lists_fwd and gnnpp_filter_head_team_lists_fwd on the lists of S == the dense-S calls, byte for
    byte.  K = 1: lists NULL.  The head runs when the case's S is batched."""
    B, N, G, F, K, E = c['B'], c['N'], c['G'], c['F'], c['K'], c['E']
    batched = c.get('batched', True)
    h, S, x, b = fc.make_inputs(c['seed'], B, N, G, F, K, E, None, batched, c.get('bias'), 1.0)
    S = _s_variant(c, S)
    f64 = int(S.dtype == np.float64)
    Sd = bk.put(S)
    xb, packed = bk.put(np.ascontiguousarray(x.transpose(0, 2, 1))), fc.pack(bk, h)
    bb = bk.put(b) if b is not None else None
    lists = filter_lists(bk, S, N) if K > 1 else None
    lp = lists.ptr if lists is not None else None
    per_node, relu = int(c.get('bias') == 'node'), c.get('relu', 0)
    y0, y1 = bk.empty((B, N, F)), bk.empty((B, N, F))
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_fwd(xb.ptr, Sd.ptr, packed.ptr, bb.ptr if bb else None, y0.ptr, ws.ptr, nbytes, B, N,
                                       G, F, K, E, f64, int(batched), relu, per_node, prec, bk.stream) == 0
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, batched)
    assert bk.lib.gnnpp_lsigf_team_lists_fwd(xb.ptr, lp, packed.ptr, bb.ptr if bb else None, y1.ptr, ws.ptr, nbytes, B,
                                             N, G, F, K, E, int(batched), relu, per_node, prec, bk.stream) == 0
    bk.sync()
    a0, a1 = y0.get(), y1.get()
    assert np.isfinite(a0).all() and a0.tobytes() == a1.tobytes(), c['name']
    if K > 1:                                        # the lists region of the workspace went unused
        li = layout((B if batched else 1) * E, N)[3]
        assert np.isnan(ws.get()[:li // 4]).all(), c['name']
    if not batched or per_node:
        return
    g = np.random.default_rng(c['seed'] + 2)
    aw = bk.put((g.standard_normal((5, F)) / np.sqrt(F / 2.0)).astype(np.float32))
    ab = bk.put(g.standard_normal(5).astype(np.float32))
    l0, l1 = bk.empty((N, B, 5)), bk.empty((N, B, 5))
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, True)
    assert bk.lib.gnnpp_filter_head_team_fwd(xb.ptr, Sd.ptr, packed.ptr, bb.ptr if bb else None, aw.ptr, ab.ptr, l0.ptr,
                                             ws.ptr, nbytes, B, N, G, F, K, E, f64, prec, bk.stream) == 0
    ws, nbytes = tc.workspace(bk, B, N, G, K, E, True)
    assert bk.lib.gnnpp_filter_head_team_lists_fwd(xb.ptr, lp, packed.ptr, bb.ptr if bb else None, aw.ptr, ab.ptr, l1.ptr,
                                                   ws.ptr, nbytes, B, N, G, F, K, E, prec, bk.stream) == 0
    bk.sync()
    a0, a1 = l0.get(), l1.get()
    assert np.isfinite(a0).all() and a0.tobytes() == a1.tobytes(), c['name'] + '/head'


def run_policy_equal(bk, B, N, K, prec, seed, s=None):
    """gnnpp_policy_team_lists_fwd on the lists of S == gnnpp_policy_team_fwd on S, byte for byte (G = F = 128)."""
    import policy_f64_cases as pc
    from oracle import policy_oracle as orc
    sd = orc.init_state_dict(K, seed=seed)
    obs = orc.synth_obs(B, N, seed=seed + 1)
    _, S, _, _ = fc.make_inputs(seed, B, N, 128, 128, K, 1)
    S = tc.shape_s(S, s, seed)
    enc, filt = pc.pack_encoder(bk, sd), pc.pack_filter(bk, sd['GFL.0.weight'].numpy())
    ob = bk.put(np.ascontiguousarray(obs.numpy(), np.float32))
    gb, aw, ab = (bk.put(np.ascontiguousarray(sd[k].numpy().reshape(-1), np.float32))
                  for k in ('GFL.0.bias', 'actionsMLP.0.weight', 'actionsMLP.0.bias'))
    Sd = bk.put(S)
    lists = filter_lists(bk, S, N) if K > 1 else None
    out = []
    for use_lists in (False, True):
        feat, logits = bk.empty((B * N, 128)), bk.empty((N, B, 5))
        ws, nbytes = tc.workspace(bk, B, N, 128, K, 1, True)
        if use_lists:
            rc = bk.lib.gnnpp_policy_team_lists_fwd(ob.ptr, lists.ptr if lists is not None else None, enc.ptr, filt.ptr,
                                                    gb.ptr, aw.ptr, ab.ptr, feat.ptr, logits.ptr, B, N, K, 1, prec, None,
                                                    bk.stream, ws.ptr, nbytes)
        else:
            rc = bk.lib.gnnpp_policy_team_fwd(ob.ptr, Sd.ptr, enc.ptr, filt.ptr, gb.ptr, aw.ptr, ab.ptr, feat.ptr,
                                              logits.ptr, B, N, K, 1, 0, prec, None, bk.stream, ws.ptr, nbytes)
        assert rc == 0, rc
        bk.sync()
        out.append(logits.get())
    assert np.isfinite(out[0]).all() and out[0].tobytes() == out[1].tobytes()


def run_filter_errors(bk):
    """The error table of the three lists calls: the code, and output + workspace (pre-filled with NaN) untouched."""
    B, N, G, F, K, E = 1, 20, 24, 24, 3, 1
    h, S, x, _ = fc.make_inputs(5, B, N, G, F, K, E)
    xb, packed = bk.put(np.ascontiguousarray(x.transpose(0, 2, 1))), fc.pack(bk, h)
    lists = filter_lists(bk, S, N)
    lists1k = bk.put(np.zeros(bk.lib.gnnpp_team_lists_bytes(1, 1024) + 16, np.uint8))
    aw, ab = bk.put(np.ones((5, F), np.float32)), bk.put(np.ones(5, np.float32))
    big = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, 1024, 128, K, E, 1)
    need = bk.lib.gnnpp_lsigf_team_workspace_bytes(B, N, G, K, E, 1)
    off = lambda buf, n: ctypes.c_void_p(buf.ptr.value + n)                    # noqa: E731

    def fwd(y, ws, nbytes, lp=lists.ptr, N=N, G=G, F=F, prec=0, x=xb.ptr, pk=packed.ptr, wsoff=0):
        return bk.lib.gnnpp_lsigf_team_lists_fwd(x, lp, pk, None, y.ptr if y else None, off(ws, wsoff), nbytes, B, N, G,
                                                 F, K, E, 1, 0, 0, prec, bk.stream)

    def head(y, ws, nbytes, lp=lists.ptr, prec=0, aw=aw.ptr, F=F):
        return bk.lib.gnnpp_filter_head_team_lists_fwd(xb.ptr, lp, packed.ptr, None, aw, ab.ptr, y.ptr, ws.ptr, nbytes,
                                                       B, N, G, F, K, E, prec, bk.stream)

    def policy(y, ws, nbytes, lp=lists1k.ptr, prec=0, N=1024, obs=xb.ptr):
        return bk.lib.gnnpp_policy_team_lists_fwd(obs, lp, packed.ptr, packed.ptr, None, aw.ptr, ab.ptr, xb.ptr, y.ptr,
                                                  B, N, K, E, prec, None, bk.stream, ws.ptr, nbytes)

    table = (('NULL lists at K = 3', fwd, dict(lp=None), big, ERR_ARG),
             ('misaligned lists', fwd, dict(lp=off(lists, 8)), big, ERR_ARG),
             ('NULL x', fwd, dict(x=None), big, ERR_ARG), ('NULL taps', fwd, dict(pk=None), big, ERR_ARG),
             ('N = 1025', fwd, dict(N=1025), big, ERR_ARG), ('N = 0', fwd, dict(N=0), big, ERR_ARG),
             ('precision 3', fwd, dict(prec=3), big, ERR_ARG), ('short workspace', fwd, {}, need - 1, ERR_ARG),
             ('misaligned workspace', fwd, dict(wsoff=4), need, ERR_ARG),
             ('G = 129', fwd, dict(G=129), big, ERR_UNSUPPORTED), ('F = 129', fwd, dict(F=129), big, ERR_UNSUPPORTED),
             ('split-f16', fwd, dict(prec=2), big, ERR_UNSUPPORTED),
             ('head: NULL lists', head, dict(lp=None), big, ERR_ARG), ('head: NULL act_w', head, dict(aw=None), big, ERR_ARG),
             ('head: misaligned lists', head, dict(lp=off(lists, 4)), big, ERR_ARG),
             ('head: split-f16', head, dict(prec=2), big, ERR_UNSUPPORTED),
             ('head: F = 129', head, dict(F=129), big, ERR_UNSUPPORTED),
             ('policy: NULL lists', policy, dict(lp=None), big, ERR_ARG), ('policy: NULL obs', policy, dict(obs=None), big, ERR_ARG),
             ('policy: misaligned lists', policy, dict(lp=off(lists1k, 8)), big, ERR_ARG),
             ('policy: N = 1025', policy, dict(N=1025), big, ERR_ARG), ('policy: short workspace', policy, {}, big - 16, ERR_ARG),
             ('policy: split-f16', policy, dict(prec=2), big, ERR_UNSUPPORTED))
    for name, fn, kw, nbytes, code in table:
        y = bk.empty((B, 1025, 129))
        ws = bk.put(np.full(big // 4 + 4, np.nan, np.float32))
        assert fn(y, ws, nbytes, **kw) == code, name
        bk.sync()
        assert np.isnan(y.get()).all() and np.isnan(ws.get()).all(), name
    ws = bk.put(np.full(big // 4, np.nan, np.float32))
    assert fwd(None, ws, big) == ERR_ARG
    bk.sync()
    assert np.isnan(ws.get()).all()
    # ... and the call itself works with exactly the bytes it asks for
    y = bk.empty((B, N, F))
    ws = bk.put(np.full(need // 4, np.nan, np.float32))
    assert fwd(y, ws, need) == 0
    bk.sync()
    assert np.isfinite(y.get()).all()
    assert bk.lib.gnnpp_version() == 330


FILTER_CASES = [
    dict(name='N20/K2/G24F24/unsym', seed=21, B=2, N=20, G=24, F=24, K=2, E=1, bias='feat'),
    dict(name='N20/K4/G24F24/full_empty/relu', seed=22, B=2, N=20, G=24, F=24, K=4, E=1, bias='feat', relu=1,
         s='full_empty'),
    dict(name='N20/K1/G24F24/nullLists', seed=23, B=2, N=20, G=24, F=24, K=1, E=1, bias='feat'),
    dict(name='N20/K4E2/G24F24/sharedS/node/f64S', seed=24, B=2, N=20, G=24, F=24, K=4, E=2, bias='node', batched=False,
         f64=1),
    dict(name='N130/K2E2/G128F128/unsym', seed=25, B=1, N=130, G=128, F=128, K=2, E=2, bias='feat'),
    dict(name='N130/K4/G128F128/full_empty', seed=26, B=2, N=130, G=128, F=128, K=4, E=1, s='full_empty', relu=1),
    dict(name='N130/K1/G128F128/nullLists', seed=27, B=1, N=130, G=128, F=128, K=1, E=1, bias='feat'),
    dict(name='N130/K2/G128F128/sharedS/sym', seed=28, B=2, N=130, G=128, F=128, K=2, E=1, batched=False, s='sym'),
]
GPU_FILTER_CASES = [
    dict(name='B2N1024/K4/G128F128/full_empty', seed=31, B=2, N=1024, G=128, F=128, K=4, E=1, bias='feat', relu=1,
         s='full_empty'),
    dict(name='B2N1024/K2E2/G128F128/sharedS/f64S', seed=32, B=2, N=1024, G=128, F=128, K=2, E=2, batched=False, f64=1),
]

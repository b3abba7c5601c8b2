"""The five launches of csrc/train_ops.hip through the C ABI (gnnpp_gemm_kmajor, gnnpp_gemm_kmajor_multi,
gnnpp_linear_fwd, gnnpp_policy_loss, gnnpp_adam_step): case tables, float64 statements and runners, shared by
tests/test_emu_train_ops.py (host emulation, a reduced matrix) and tests/test_gpu_train_ops.py (MI355X).  A plain
helper module, not a conftest.

Every floating result is held to a float64 numpy statement of the operation on the fp32 inputs, with the same statement
in fp32 on the CPU as the measure (f64_yardstick.gap, its constants unchanged): numpy `@`, torch's cross_entropy,
torch.optim.Adam(foreach=False).  Every output lives in a buffer filled with a NaN of a known payload with MARGIN
floats of it on either side: whatever the call does not address (the gaps of a strided C included) must keep those
bits.  Every call is made twice and must return the same bytes (the launches are deterministic).

gemm_plan (train_ops.hip) is restated here (`gemm_plan`) so that the table can assert, on the CPU, which split counts
it reaches; test_*_gemm_plan_is_the_library's holds the restatement to gnnpp_gemm_workspace_floats for every case.  The
shape sets the cases draw from cannot reach ksplit = 5 (no tile count of 52 .. 63, no K of 129 .. 160 among them): one
case uses K = 150 for it.
"""
import ctypes

import numpy as np

from f64_yardstick import ULP, gap
from gnn_pathplanning_amd._native import ERR_ARG, ERR_UNSUPPORTED, AdamTensors, GemmDesc

MARGIN = 64                                   # floats on either side of every output (a multiple of 4: 16-byte alignment)
SENT_BITS = 0x7FC5A5A5                        # a quiet NaN with a payload no arithmetic produces
SENT = np.array([SENT_BITS], np.uint32).view(np.float32)[0]


# ---- guarded buffers ---------------------------------------------------------------------------------------------
class Guarded:
    """n floats the call may write, MARGIN sentinel floats on either side; `init` (n floats) or the sentinel inside."""

    def __init__(self, bk, n, init=None):
        flat = np.full(n + 2 * MARGIN, SENT, np.float32)
        if init is not None:
            flat[MARGIN:MARGIN + n] = np.ravel(init)
        self.n, self.buf = n, bk.put(flat)
        self.ptr = ctypes.c_void_p(self.buf.ptr.value + 4 * MARGIN)

    def at(self, floats):
        return ctypes.c_void_p(self.ptr.value + 4 * floats)

    def bits(self):
        return self.buf.get().view(np.uint32)

    def read(self, name, idx=None):
        """The floats at offsets idx (all n when None); everything else must still be the sentinel."""
        a = self.bits()
        own = np.zeros(a.size, bool)
        own[MARGIN + (np.arange(self.n) if idx is None else np.ravel(idx))] = True
        assert (a[~own] == SENT_BITS).all(), '%s: wrote outside what the call addresses' % name
        out = a.view(np.float32)[MARGIN:MARGIN + self.n]
        return out.copy() if idx is None else out[idx]

    def untouched(self):
        return bool((self.bits() == SENT_BITS).all())


def check(name, got, want64, ref32, scale=None):
    ok, rep = gap(got, want64, ref32, scale)
    assert ok, '%s: %s' % (name, {k: '%.3g' % v for k, v in rep.items()})
    return rep


def same_bits(name, a, b):
    assert np.asarray(a, np.float32).view(np.uint32).tobytes() == np.asarray(b, np.float32).view(np.uint32).tobytes(), name


# ---- gemm_kmajor -------------------------------------------------------------------------------------------------
def gemm_plan(batch, M, N, K):
    """(ksplit, kper) of train_ops.hip gemm_plan."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * batch
    ks = max(1, min((256 + tiles - 1) // tiles, (K + 31) // 32))
    kper = (((K + ks - 1) // ks) + 3) // 4 * 4
    return (K + kper - 1) // kper, kper


def workspace_floats(batch, M, N, K):
    ks = gemm_plan(batch, M, N, K)[0]
    return (ks * batch * M * N + 3) // 4 * 4 if ks > 1 else 0


def _g(i, batch, M, N, K, a='contig', b='contig', c='contig', scale=1.0):
    return dict(name='b%d/%dx%dx%d/A=%s/B=%s/C=%s/x%g' % (batch, M, N, K, a, b, c, scale), seed=300 + i, batch=batch, M=M,
                N=N, K=K, a=a, b=b, c=c, scale=scale)


# A: contig [b][m][k] | trans [b][k][m] (a_sm = 1, a_sk = M) | shared (a_sb = 0) | row (a_sm = 0, M = 1: the ones row of a
# bias gradient, with random entries);  B: contig [b][k][n] | shared (b_sb = 0);  C: contig | pad (c_sm = N + 3) | inter
# ([m][b][n]: the layout of the tap gradient dh)
GEMM_CASES = [
    _g(0, 1, 1, 1, 1), _g(1, 1, 15, 5, 3), _g(2, 1, 16, 15, 4, a='trans'), _g(3, 1, 17, 17, 5, c='pad'),
    _g(4, 3, 63, 63, 31, a='shared', c='inter'), _g(5, 1, 64, 64, 32, a='trans'), _g(6, 1, 65, 65, 33),
    _g(7, 12, 1, 130, 64, a='row'), _g(8, 1, 130, 1, 65, c='pad'), _g(9, 3, 17, 63, 70, a='trans', b='shared', c='inter'),
    _g(10, 12, 65, 130, 300, a='shared', c='inter'), _g(11, 1, 16, 64, 150), _g(12, 3, 130, 130, 300),
    _g(13, 1, 1, 5, 300, a='row'), _g(14, 1, 5, 130, 300, a='trans'), _g(15, 1, 63, 64, 64, b='shared', c='pad'),
    _g(16, 3, 15, 17, 33, c='inter'), _g(17, 1, 17, 1, 1), _g(18, 12, 16, 15, 4, a='shared', b='shared'),
    _g(19, 1, 64, 65, 70, scale=1e-18), _g(20, 3, 65, 63, 70, c='inter', scale=1e18),
    _g(21, 1, 130, 15, 31, a='trans', c='pad'), _g(22, 1, 17, 130, 3), _g(23, 3, 1, 15, 5, a='row', c='inter'),
    _g(24, 1, 15, 17, 32), _g(25, 12, 63, 5, 65), _g(26, 1, 65, 1, 300, a='trans'), _g(27, 1, 16, 17, 64),
    _g(28, 3, 64, 5, 65, a='trans', c='pad'),
]
GPU_GEMM_CASES = [_g(40, 1, 130, 130, 5120, a='trans'), _g(41, 1, 64, 17, 5120, b='shared', c='pad')]
EMU_GEMM_CASES = GEMM_CASES


def _gemm_coverage(cases):
    plans = [gemm_plan(c['batch'], c['M'], c['N'], c['K']) for c in cases]
    splits = {p[0] for p in plans}
    assert {1, 2, 3, 4, 5} <= splits and max(splits) >= 9, sorted(splits)
    assert any(ks > 1 and c['K'] % kper for c, (ks, kper) in zip(cases, plans))      # a last split shorter than kper
    for key, values in (('M', (1, 15, 16, 17, 63, 64, 65, 130)), ('N', (1, 5, 15, 17, 63, 64, 65, 130)),
                        ('batch', (1, 3, 12)), ('a', ('contig', 'trans', 'shared', 'row')), ('b', ('contig', 'shared')),
                        ('c', ('contig', 'pad', 'inter')), ('scale', (1.0, 1e-18, 1e18))):
        assert set(values) <= {c[key] for c in cases}, key
    # a split product in every C layout, and one with batch > 1
    assert {'contig', 'pad', 'inter'} <= {c['c'] for c, p in zip(cases, plans) if p[0] > 1}
    assert any(p[0] > 1 and c['batch'] > 1 for c, p in zip(cases, plans))


_gemm_coverage(EMU_GEMM_CASES)
assert {1, 3, 4, 5, 31, 32, 33, 64, 65, 70, 300} <= {c['K'] for c in EMU_GEMM_CASES}
assert 5120 in {c['K'] for c in GPU_GEMM_CASES} and 5120 not in {c['K'] for c in EMU_GEMM_CASES}
assert any((c['M'], c['N'], c['K'], c['batch']) == (130, 130, 5120, 1) for c in GPU_GEMM_CASES)


class Product:
    """Operands of one case on the backend, the logical A [b,M,K] and B [b,K,N], C's strides and addressed offsets."""

    def __init__(self, bk, c):
        batch, M, N, K = c['batch'], c['M'], c['N'], c['K']
        g = np.random.default_rng(c['seed'])
        s = np.float32(c['scale'])
        self.c, self.dims = c, (batch, M, N, K)
        if c['a'] == 'row':
            assert M == 1
            store = (g.standard_normal(K).astype(np.float32) * s)
            self.A, self.a_st = np.broadcast_to(store.reshape(1, 1, K), (batch, 1, K)), (0, 0, 1)
        elif c['a'] == 'shared':
            store = g.standard_normal((M, K)).astype(np.float32) * s
            self.A, self.a_st = np.broadcast_to(store, (batch, M, K)), (0, K, 1)
        elif c['a'] == 'trans':
            store = g.standard_normal((batch, K, M)).astype(np.float32) * s
            self.A, self.a_st = store.transpose(0, 2, 1), (M * K, 1, M)
        else:
            store = g.standard_normal((batch, M, K)).astype(np.float32) * s
            self.A, self.a_st = store, (M * K, K, 1)
        self.a_buf = bk.put(store)
        if c['b'] == 'shared':
            storeb = g.standard_normal((K, N)).astype(np.float32) * s
            self.B, self.b_st = np.broadcast_to(storeb, (batch, K, N)), (0, N)
        else:
            storeb = g.standard_normal((batch, K, N)).astype(np.float32) * s
            self.B, self.b_st = storeb, (K * N, N)
        self.b_buf = bk.put(storeb)
        if c['c'] == 'pad':
            self.c_st = (M * (N + 3), N + 3)
        elif c['c'] == 'inter':
            self.c_st = (N, batch * N)
        else:
            self.c_st = (M * N, N)
        b_, m_, n_ = np.meshgrid(np.arange(batch), np.arange(M), np.arange(N), indexing='ij')
        self.idx = b_ * self.c_st[0] + m_ * self.c_st[1] + n_                     # [b,M,N] offsets into C
        self.span = int(self.idx.max()) + 1
        assert np.unique(self.idx).size == self.idx.size

    def want(self, dt):
        return np.matmul(self.A.astype(dt), self.B.astype(dt))

    def desc(self, d, C, mask=None):
        batch, M, N, K = self.dims
        d.A, (d.a_sb, d.a_sm, d.a_sk) = self.a_buf.ptr, self.a_st
        d.B, (d.b_sb, d.b_sk) = self.b_buf.ptr, self.b_st
        d.C, (d.c_sb, d.c_sm) = C.ptr, self.c_st
        d.batch, d.M, d.N, d.K = batch, M, N, K
        d.mask = mask.ptr if mask is not None else None

    def alone(self, bk):
        """gnnpp_gemm_kmajor of this product into a fresh guarded C; the workspace has exactly the floats asked for."""
        batch, M, N, K = self.dims
        nws = bk.lib.gnnpp_gemm_workspace_floats(batch, M, N, K)
        ws = Guarded(bk, nws)
        C = Guarded(bk, self.span)
        rc = bk.lib.gnnpp_gemm_kmajor(self.a_buf.ptr, *self.a_st, self.b_buf.ptr, *self.b_st, C.ptr, *self.c_st, batch, M, N,
                                      K, ws.ptr if nws else None, bk.stream)
        assert rc == 0, (self.c['name'], rc)
        bk.sync()
        ws.read(self.c['name'] + '/workspace')
        return C.read(self.c['name'], self.idx)


def run_gemm_plan(bk, cases):
    """The restated plan against the library: the workspace of every case is ksplit * batch * M * N floats rounded up to
    4, or 0 when the contraction is not split."""
    for c in cases:
        dims = (c['batch'], c['M'], c['N'], c['K'])
        assert bk.lib.gnnpp_gemm_workspace_floats(*dims) == workspace_floats(*dims), c['name']
    assert bk.lib.gnnpp_gemm_workspace_floats(0, 4, 4, 4) == 0 and bk.lib.gnnpp_gemm_workspace_floats(1, 4, 4, 0) == 0


def run_gemm(bk, c):
    p = Product(bk, c)
    got, again = p.alone(bk), p.alone(bk)
    same_bits(c['name'] + '/twice', got, again)
    return check(c['name'], got, p.want(np.float64), p.want(np.float32))


# ---- gemm_kmajor_multi -------------------------------------------------------------------------------------------
MULTI_CASES = [
    _g(50, 1, 63, 130, 5, c='pad'),                               # dx of a Linear: unsplit, c_sm > N
    _g(51, 1, 5, 130, 70, a='trans'),                             # dW: split
    _g(52, 3, 17, 15, 33, a='shared', c='inter'),                 # split, batch > 1, C interleaved
    _g(53, 1, 1, 5, 70, a='row'),                                 # db: split
    _g(54, 1, 64, 64, 32),                                        # unsplit
    _g(55, 1, 65, 17, 300, a='trans', c='pad'),                   # split, c_sm > N
    _g(56, 12, 16, 5, 4, a='shared', c='inter'),                  # unsplit, batch > 1, C interleaved
    _g(57, 1, 130, 65, 65),                                       # split
]
MULTI_MASKED = ((0, 2), (5, 6))                                   # two masked products per call; both calls are made
_mp = [gemm_plan(c['batch'], c['M'], c['N'], c['K'])[0] for c in MULTI_CASES]
assert len(MULTI_CASES) == 8 and 1 in _mp and max(_mp) > 1
assert {(_mp[i] > 1, MULTI_CASES[i]['c']) for pair in MULTI_MASKED for i in pair} == \
    {(False, 'pad'), (True, 'inter'), (True, 'pad'), (False, 'inter')}
MASK_EDGES = np.array([0x00000000, 0x80000000, 0x80011111, 0x7FC00000, 0xFFC00000, 0x00011111],
                      np.uint32).view(np.float32)     # +0, -0, a negative denormal, NaN, -NaN: store 0; a positive denormal: keep


def _mask(seed, span, idx):
    """A mask laid out like C: normal values, and the edge values spread over the ADDRESSED entries."""
    g = np.random.default_rng(seed)
    m = g.standard_normal(span).astype(np.float32)
    flat = np.ravel(idx)
    where = flat[g.permutation(flat.size)[:min(flat.size, 4 * MASK_EDGES.size)]]
    m[where] = np.resize(MASK_EDGES, where.size)
    return m


def run_gemm_multi(bk):
    """Eight products in one call: each result has the bits of the same product run alone through gnnpp_gemm_kmajor
    (the same plan, so the same summation order), the masked ones those of np.where(mask > 0, alone, 0)."""
    prods = [Product(bk, c) for c in MULTI_CASES]
    alone = [p.alone(bk) for p in prods]
    for p, a in zip(prods, alone):
        check(p.c['name'], a, p.want(np.float64), p.want(np.float32))
    for masked in MULTI_MASKED:
        outs = []
        for rep in range(2):
            arr = (GemmDesc * 8)()
            Cs = [Guarded(bk, p.span) for p in prods]
            masks = {i: _mask(prods[i].c['seed'], prods[i].span, prods[i].idx) for i in masked}
            mbufs = {i: bk.put(masks[i]) for i in masked}
            for i, p in enumerate(prods):
                p.desc(arr[i], Cs[i], mbufs.get(i))
            nws = bk.lib.gnnpp_gemm_multi_workspace_floats(arr, 8)
            assert nws == sum(workspace_floats(*p.dims) for p in prods)
            ws = Guarded(bk, nws)
            assert bk.lib.gnnpp_gemm_kmajor_multi(arr, 8, ws.ptr, bk.stream) == 0
            bk.sync()
            ws.read('multi/workspace')
            outs.append([C.read(p.c['name'], p.idx) for C, p in zip(Cs, prods)])
        for i, p in enumerate(prods):
            name = 'multi%s/%d/%s' % (masked, i, p.c['name'])
            same_bits(name + '/twice', outs[0][i], outs[1][i])
            if i in masked:
                keepm = masks[i][p.idx] > 0
                assert 0 < keepm.sum() < keepm.size
                same_bits(name + '/masked', outs[0][i], np.where(keepm, alone[i], np.float32(0)))
            else:
                same_bits(name, outs[0][i], alone[i])


def run_gemm_errors(bk):
    """The refusals of gnnpp_api.hip (all GNNPP_ERR_ARG); a refusal launches nothing: C keeps the sentinel."""
    prods = [Product(bk, MULTI_CASES[i]) for i in (1, 4)]                  # one split, one not
    nws = sum(workspace_floats(*p.dims) for p in prods)
    assert nws > 0

    def call(count=2, null=None, field=None, value=0, ws=True, use=2):
        arr = (GemmDesc * 9)()
        Cs = [Guarded(bk, p.span) for p in prods]
        for i in range(9):
            prods[i % 2].desc(arr[i], Cs[i % 2])
        if field:
            setattr(arr[use - 1], field, value)
        w = Guarded(bk, nws)
        rc = bk.lib.gnnpp_gemm_kmajor_multi(None if null else arr, count, w.ptr if ws else None, bk.stream)
        bk.sync()
        return rc, all(C.untouched() for C in Cs) and w.untouched()

    table = (('count 9', dict(count=9)), ('count 0', dict(count=0)), ('count -1', dict(count=-1)),
             ('NULL descriptors', dict(null=True)), ('NULL A', dict(field='A', value=None)),
             ('NULL B', dict(field='B', value=None)), ('NULL C', dict(field='C', value=None)),
             ('batch 0', dict(field='batch')), ('M 0', dict(field='M')), ('N 0', dict(field='N')), ('K 0', dict(field='K')),
             ('NULL workspace of a split product', dict(ws=False)))
    for name, kw in table:
        rc, clean = call(**kw)
        assert rc == ERR_ARG and clean, (name, rc, clean)
    p = prods[0]
    C = Guarded(bk, p.span)
    batch, M, N, K = p.dims
    for name, args in (('NULL A', (None, p.b_buf.ptr, C.ptr, K)), ('NULL B', (p.a_buf.ptr, None, C.ptr, K)),
                       ('NULL C', (p.a_buf.ptr, p.b_buf.ptr, None, K)), ('K 0', (p.a_buf.ptr, p.b_buf.ptr, C.ptr, 0))):
        A_, B_, C_, K_ = args
        w = Guarded(bk, nws)
        assert bk.lib.gnnpp_gemm_kmajor(A_, *p.a_st, B_, *p.b_st, C_, *p.c_st, batch, M, N, K_, w.ptr, bk.stream) == ERR_ARG, name
        bk.sync()
        assert C.untouched() and w.untouched(), name
    rc, clean = call()                                                          # ... and the table's own call is accepted
    assert rc == 0 and not clean


# ---- linear_fwd --------------------------------------------------------------------------------------------------
def _l(i, R, O, I, relu, bias):
    return dict(name='R%d/O%d/I%d/relu%d/%s' % (R, O, I, relu, 'bias' if bias else 'nobias'), seed=400 + i, R=R, O=O, I=I,
                relu=relu, bias=bias)


LINEAR_CASES = [
    _l(0, 1, 1, 64, 0, True), _l(1, 15, 3, 128, 1, True), _l(2, 16, 4, 192, 0, False), _l(3, 17, 5, 256, 1, True),
    _l(4, 37, 6, 64, 1, False), _l(5, 640, 16, 128, 0, True), _l(6, 37, 17, 128, 1, True), _l(7, 16, 20, 192, 0, True),
    _l(8, 17, 128, 128, 1, True), _l(9, 15, 130, 256, 0, False), _l(10, 640, 5, 128, 0, True), _l(11, 1, 130, 64, 1, True),
    _l(12, 37, 128, 256, 0, False), _l(13, 16, 16, 64, 1, True), _l(14, 17, 17, 192, 1, True), _l(15, 640, 3, 64, 1, False),
]
EMU_LINEAR_CASES = LINEAR_CASES
assert {c['R'] for c in LINEAR_CASES} == {1, 15, 16, 17, 37, 640} and {c['I'] for c in LINEAR_CASES} == {64, 128, 192, 256}
assert {c['O'] for c in LINEAR_CASES} == {1, 3, 4, 5, 6, 16, 17, 20, 128, 130}
assert sum((((c['R'] + 15) // 16) * ((c['O'] + 15) // 16)) % 4 != 0 for c in LINEAR_CASES) >= 2   # waves that return early
assert {(c['relu'], c['bias']) for c in LINEAR_CASES} == {(0, True), (0, False), (1, True), (1, False)}


def _linear(x, W, b, relu, dt):
    y = x.astype(dt) @ W.astype(dt).T
    if b is not None:
        y = y + b.astype(dt)
    return np.maximum(y, 0) if relu else y


def _linear_call(bk, x, W, b, relu, name):
    R, I = x.shape
    O = W.shape[0]
    xb, Wb, bb = bk.put(x), bk.put(W), (bk.put(b) if b is not None else None)
    outs = []
    for _ in range(2):
        y = Guarded(bk, R * O)
        assert xb.ptr.value % 16 == 0 and Wb.ptr.value % 16 == 0 and y.ptr.value % 16 == 0
        assert bk.lib.gnnpp_linear_fwd(xb.ptr, Wb.ptr, bb.ptr if bb else None, y.ptr, R, I, O, relu, bk.stream) == 0, name
        bk.sync()
        outs.append(y.read(name).reshape(R, O))
    same_bits(name + '/twice', outs[0], outs[1])
    return outs[0]


def run_linear(bk, c):
    R, O, I, relu = c['R'], c['O'], c['I'], c['relu']
    g = np.random.default_rng(c['seed'])
    x = g.standard_normal((R, I)).astype(np.float32)
    W = (g.standard_normal((O, I)) / np.sqrt(I)).astype(np.float32)
    b = g.standard_normal(O).astype(np.float32) if c['bias'] else None
    got = _linear_call(bk, x, W, b, relu, c['name'])
    return check(c['name'], got, _linear(x, W, b, relu, np.float64), _linear(x, W, b, relu, np.float32))


def run_linear_relu_zero(bk):
    """Small-integer operands: every product and partial sum is exact whatever the order.  The bias cancels row 2's
    pre-activations exactly: that row is +0 after the ReLU, and the whole result IS the float64 statement."""
    R, O, I = 17, 20, 64
    g = np.random.default_rng(77)
    x = g.integers(-3, 4, (R, I)).astype(np.float32)
    W = g.integers(-3, 4, (O, I)).astype(np.float32)
    b = -(x[2].astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    got = _linear_call(bk, x, W, b, 1, 'relu at exactly 0')
    want = _linear(x, W, b, 1, np.float64)
    assert (want[2] == 0).all() and (want > 0).any() and (got[2].view(np.uint32) == 0).all()
    assert np.array_equal(got.astype(np.float64), want)


def run_linear_errors(bk):
    """I = 100; x, W one float off 16-byte alignment; y one float off it where rows are stored as 16-byte vectors
    (O % 4 == 0): GNNPP_ERR_UNSUPPORTED and y untouched.  A misaligned 16-byte store is never launched.  With O % 4 != 0
    the rows are stored float by float: any y is served."""
    R, I, O = 17, 128, 4
    g = np.random.default_rng(78)
    x, W = g.standard_normal((R, I + 1)).astype(np.float32), g.standard_normal((8, I + 1)).astype(np.float32)
    xb, Wb = bk.put(np.ravel(x)), bk.put(np.ravel(W))
    off = lambda p, n: ctypes.c_void_p(p.value + 4 * n)                       # noqa: E731
    table = (('I = 100', dict(I=100), ERR_UNSUPPORTED), ('x + 1', dict(x=off(xb.ptr, 1)), ERR_UNSUPPORTED),
             ('W + 1', dict(W=off(Wb.ptr, 1)), ERR_UNSUPPORTED), ('y + 1, O = 4', dict(yoff=1), ERR_UNSUPPORTED),
             ('y + 2, O = 8', dict(yoff=2, O=8), ERR_UNSUPPORTED), ('NULL x', dict(x=None), ERR_ARG),
             ('NULL W', dict(W=None), ERR_ARG), ('NULL y', dict(yoff=None), ERR_ARG), ('R = 0', dict(R=0), ERR_ARG),
             ('O = 0', dict(O=0), ERR_ARG), ('I = 0', dict(I=0), ERR_ARG))
    for name, kw, code in table:
        y = Guarded(bk, R * 8 + 4)
        yoff = kw.get('yoff', 0)
        rc = bk.lib.gnnpp_linear_fwd(kw.get('x', xb.ptr), kw.get('W', Wb.ptr), None, None if yoff is None else y.at(yoff),
                                     kw.get('R', R), kw.get('I', I), kw.get('O', O), 0, bk.stream)
        bk.sync()
        assert rc == code and y.untouched(), (name, rc)
    O = 5                                                                        # scalar stores: y + 1 is served
    x2, W2 = np.ascontiguousarray(x[:, :I]), np.ascontiguousarray(W[:O, :I])
    xb2, Wb2 = bk.put(x2), bk.put(W2)
    y = Guarded(bk, R * O + 1)
    assert bk.lib.gnnpp_linear_fwd(xb2.ptr, Wb2.ptr, None, y.at(1), R, I, O, 0, bk.stream) == 0
    bk.sync()
    got = y.read('y + 1, O = 5', 1 + np.arange(R * O)).reshape(R, O)
    check('y + 1, O = 5', got, _linear(x2, W2, None, 0, np.float64), _linear(x2, W2, None, 0, np.float32))


# ---- policy_loss -------------------------------------------------------------------------------------------------
def _p(i, B, N, C, rows='all'):
    return dict(name='B%dxN%d/C%d/%s' % (B, N, C, rows), seed=500 + i, B=B, N=N, C=C, rows=rows)


# B * N = 1, 1023, 1024, 1025 (one more row than the workgroup has threads), 3000; rows: 'all' = every kind of logit and
# target row below, 'moderate' = without the rows holding +1e4 (whose loss of ~1e4 sets the scale of the mean)
LOSS_CASES = [
    _p(0, 1, 1, 5), _p(1, 1, 1, 1), _p(2, 93, 11, 5), _p(3, 64, 16, 2), _p(4, 41, 25, 7), _p(5, 300, 10, 5),
    _p(6, 3, 5, 64), _p(7, 33, 31, 64, 'moderate'), _p(8, 205, 5, 5, 'moderate'), _p(9, 31, 33, 1), _p(10, 1, 1, 64, 'moderate'),
]
EMU_LOSS_CASES = [c for c in LOSS_CASES if c['B'] * c['N'] != 3000]
assert {c['B'] * c['N'] for c in LOSS_CASES} >= {1, 1023, 1024, 1025, 3000} and {c['C'] for c in LOSS_CASES} == {1, 2, 5, 7, 64}
assert {c['B'] * c['N'] for c in EMU_LOSS_CASES} >= {1, 1023, 1024, 1025}


def loss_inputs(c):
    """logits [N,B,C] (agent-major), target [B,N,C].  Row r = n B + b takes logit kind r % 5 (3 randn | all equal | +-80
    mixed | one entry +1e4 with the label on it | ... with the label off it) and target kind (r // 5) % 5 (one-hot | a
    tie of two maxima: the first wins | soft | all zero: label 0 | all negative); the +1e4 rows take a one-hot target
    that puts the label where the kind says."""
    B, N, C = c['B'], c['N'], c['C']
    g = np.random.default_rng(c['seed'])
    lg = np.zeros((N, B, C), np.float32)
    tg = np.zeros((B, N, C), np.float32)
    kinds = 5 if c['rows'] == 'all' else 3
    for r in range(N * B):
        n, b = divmod(r, B)
        lk, tk = r % kinds, (r // kinds) % 5
        if lk == 0:
            lg[n, b] = 3 * g.standard_normal(C)
        elif lk == 1:
            lg[n, b] = np.float32(g.standard_normal())
        elif lk == 2:
            lg[n, b] = 80.0 * g.choice([-1.0, 1.0], C)
        else:
            lg[n, b] = 3 * g.standard_normal(C)
            big = int(g.integers(C))
            lg[n, b, big] = 1e4
            tg[b, n, big if (lk == 3 or C == 1) else (big + 1 + int(g.integers(C - 1))) % C] = 1.0
            continue
        if tk == 0:
            tg[b, n, int(g.integers(C))] = 1.0
        elif tk == 1:
            tg[b, n] = 0.25
            tg[b, n, g.permutation(C)[:2]] = 0.75
        elif tk == 2:
            tg[b, n] = g.dirichlet(np.ones(C))
        elif tk == 4:
            tg[b, n] = -1.0 - g.random(C)
    return lg, tg


def loss_statement(lg, tg, dt):
    """(loss, dlogits [N,B,C]) in numpy dtype dt: the header's formula, the label the FIRST maximum of the target row."""
    N, B, C = lg.shape
    x = lg.astype(dt)
    label = np.argmax(tg.transpose(1, 0, 2), -1)                                  # [N,B]: first maximum
    mx = x.max(-1, keepdims=True)
    e = np.exp(x - mx)
    lse = mx[..., 0] + np.log(e.sum(-1))
    picked = np.take_along_axis(x, label[..., None], -1)[..., 0]
    soft = e / e.sum(-1, keepdims=True)
    soft[np.arange(N)[:, None], np.arange(B)[None, :], label] -= 1
    return (lse - picked).mean(), soft / (N * B)


def loss_reference32(lg, tg):
    """torch.nn.functional.cross_entropy in fp32 on the CPU over all N B rows, and autograd's gradient."""
    import torch
    x = torch.from_numpy(lg.copy()).requires_grad_(True)
    label = torch.from_numpy(tg).permute(1, 0, 2).argmax(-1)
    loss = torch.nn.functional.cross_entropy(x.reshape(-1, lg.shape[-1]), label.reshape(-1))
    loss.backward()
    assert np.array_equal(label.numpy(), np.argmax(tg.transpose(1, 0, 2), -1))
    return loss.item(), x.grad.numpy()


def run_loss(bk, c):
    B, N, C = c['B'], c['N'], c['C']
    lg, tg = loss_inputs(c)
    want_loss, want_d = loss_statement(lg, tg, np.float64)
    ref_loss, ref_d = loss_reference32(lg, tg)
    tb = bk.put(tg)
    res = {}
    for layout in (0, 1):                                            # [N,B,C] | [B,N,C]: the same rows
        lb = bk.put(np.ascontiguousarray(lg.transpose(1, 0, 2)) if layout else lg)
        for with_grad in (True, False):
            for rep in range(2):
                loss, d = Guarded(bk, 1), Guarded(bk, N * B * C)
                assert bk.lib.gnnpp_policy_loss(lb.ptr, tb.ptr, loss.ptr, d.ptr if with_grad else None, B, N, C, layout,
                                                bk.stream) == 0, c['name']
                bk.sync()
                assert with_grad or d.untouched()
                dl = d.read(c['name']).reshape((B, N, C) if layout else (N, B, C)) if with_grad else None
                res[layout, with_grad, rep] = (loss.read(c['name']), dl.transpose(1, 0, 2) if layout and with_grad else dl)
    first = res[0, True, 0]
    for key, (loss, dl) in res.items():
        same_bits('%s/loss %s' % (c['name'], key), loss, first[0])
        if dl is not None:
            same_bits('%s/dlogits %s' % (c['name'], key), np.ascontiguousarray(dl), first[1])
    name = c['name']
    check(name + '/loss', first[0], [want_loss], [ref_loss], scale=max(abs(want_loss), 1.0) if want_loss == 0 else None)
    rep = check(name + '/dlogits', first[1], want_d, ref_d, scale=1.0 / (N * B) if C == 1 else None)
    rows = np.abs(first[1].astype(np.float64).sum(-1)).max()
    assert rows <= 8 * ULP / (N * B), '%s: a gradient row sums to %.3g = %.2f ulp of 1/(B N)' % (name, rows, rows * N * B / ULP)
    return rep


def run_loss_errors(bk):
    lg, tg = bk.put(np.zeros((2, 3, 65), np.float32)), bk.put(np.zeros((3, 2, 65), np.float32))
    table = (('C = 65', dict(C=65)), ('C = 0', dict(C=0)), ('B = 0', dict(B=0)), ('N = 0', dict(N=0)),
             ('NULL logits', dict(lg=None)), ('NULL target', dict(tg=None)), ('NULL loss', dict(loss=None)))
    for name, kw in table:
        loss, d = Guarded(bk, 1), Guarded(bk, 2 * 3 * 65)
        rc = bk.lib.gnnpp_policy_loss(kw.get('lg', lg.ptr), kw.get('tg', tg.ptr), kw.get('loss', loss.ptr), d.ptr,
                                      kw.get('B', 3), kw.get('N', 2), kw.get('C', 5), 0, bk.stream)
        bk.sync()
        assert rc == ERR_ARG and loss.untouched() and d.untouched(), (name, rc)


# ---- adam_step ---------------------------------------------------------------------------------------------------
NUMELS = (1, 255, 256, 1023, 1024, 1025, 4097)
LR, BETAS = 1e-3, (0.9, 0.999)


def _a(name, count, **kw):
    c = dict(name=name, seed=600 + len(name) + count, count=count, steps=4, wd=0.0, eps=1e-8, scale=1.0, betas={},
             start=0, zero=None)
    c.update(kw)
    return c


# a: consecutive steps (the factors cached in state[4..7]);  b: the betas change at step 3 (the cache is bypassed);
# c: a loaded state of which only state[0] = 9999 is set;  d: two tables per step (tick = 1, then tick = 0);
# e: weight decay and eps;  f: a tensor with zero gradient and zero moments
ADAM_CASES = [
    _a('a/1', 1), _a('a/5', 5), _a('a/32', 32), _a('a/5/scale1e-3', 5, scale=1e-3),
    _a('b/5', 5, betas={3: (0.8, 0.99)}), _a('b/32', 32, betas={3: (0.95, 0.9)}),
    _a('c/5', 5, steps=3, start=9999), _a('d/37', 37, steps=3), _a('d/64', 64, steps=2),
    _a('e/wd', 5, wd=1e-2), _a('e/eps', 5, eps=1e-3), _a('e/wd+eps', 7, wd=1e-2, eps=1e-3, scale=1e-3),
    _a('f/zero', 5, zero=2),
]
EMU_ADAM_CASES = ADAM_CASES


def _f32(v):
    return float(np.float32(v))


def adam_reference(c, p0, m0, v0, grads, dt):
    """torch.optim.Adam(foreach=False) in torch dtype dt on the fp32 gradients, with the hyperparameters as the fp32 values
    the kernel is handed: [(p, m, v) per tensor] after every step."""
    import torch
    ps = [torch.from_numpy(p).to(dt).clone().requires_grad_(True) for p in p0]
    opt = torch.optim.Adam(ps, lr=_f32(LR), betas=tuple(_f32(b) for b in BETAS), eps=_f32(c['eps']),
                           weight_decay=_f32(c['wd']), foreach=False)
    for p, m, v in zip(ps, m0, v0):
        opt.state[p] = {'step': torch.tensor(float(c['start'])), 'exp_avg': torch.from_numpy(m).to(dt).clone(),
                        'exp_avg_sq': torch.from_numpy(v).to(dt).clone()}
    out = []
    for s in range(c['steps']):
        if s + 1 in c['betas']:
            opt.param_groups[0]['betas'] = tuple(_f32(b) for b in c['betas'][s + 1])
        for p, gr in zip(ps, grads[s]):
            p.grad = torch.from_numpy(gr).to(dt)
        opt.step()
        out.append([(p.detach().numpy().copy(), opt.state[p]['exp_avg'].numpy().copy(),
                     opt.state[p]['exp_avg_sq'].numpy().copy()) for p in ps])
    return out


def adam_kernel_run(bk, c, p0, m0, v0, grads):
    """The schedule through gnnpp_adam_step, tables of at most 32 tensors; state[0] == t and state[3] == 0 after every
    call."""
    count = c['count']
    P = [Guarded(bk, a.size, a) for a in p0]
    M = [Guarded(bk, a.size, a) for a in m0]
    V = [Guarded(bk, a.size, a) for a in v0]
    st0 = np.zeros(8, np.float32)
    st0[0] = c['start']
    state = Guarded(bk, 8, st0)
    betas, out = BETAS, []
    for s in range(c['steps']):
        betas = c['betas'].get(s + 1, betas)
        G = [bk.put(gr) for gr in grads[s]]
        for k, i0 in enumerate(range(0, count, 32)):
            tb = AdamTensors()
            for i in range(i0, min(count, i0 + 32)):
                tb.p[i - i0], tb.g[i - i0], tb.m[i - i0], tb.v[i - i0] = P[i].ptr, G[i].ptr, M[i].ptr, V[i].ptr
                tb.numel[i - i0] = p0[i].size
            tb.count = min(count, i0 + 32) - i0
            assert bk.lib.gnnpp_adam_step(ctypes.byref(tb), state.ptr, LR, betas[0], betas[1], c['eps'],
                                          c['wd'], int(k == 0), bk.stream) == 0, c['name']
            bk.sync()
            stv = state.read(c['name'] + '/state')
            assert stv[0] == c['start'] + s + 1 and stv.view(np.uint32)[3] == 0, (c['name'], s, k, stv)
        out.append([(P[i].read(c['name']), M[i].read(c['name']), V[i].read(c['name'])) for i in range(count)])
    return out


def run_adam(bk, c):
    g = np.random.default_rng(c['seed'])
    sizes = [NUMELS[(i + c['count']) % len(NUMELS)] for i in range(c['count'])]
    if c['count'] >= len(NUMELS):
        assert set(sizes) == set(NUMELS)
    p0 = [(g.standard_normal(n) * c['scale']).astype(np.float32) for n in sizes]
    loaded = c['start'] > 0
    m0 = [(0.1 * g.standard_normal(n)).astype(np.float32) if loaded else np.zeros(n, np.float32) for n in sizes]
    v0 = [(0.01 * g.random(n)).astype(np.float32) if loaded else np.zeros(n, np.float32) for n in sizes]
    grads = [[g.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(c['steps'])]
    if c['zero'] is not None:
        for s in range(c['steps']):
            grads[s][c['zero']][:] = 0
    import torch
    w64, w32 = (adam_reference(c, p0, m0, v0, grads, dt) for dt in (torch.float64, torch.float32))
    got, again = adam_kernel_run(bk, c, p0, m0, v0, grads), adam_kernel_run(bk, c, p0, m0, v0, grads)
    for s in range(c['steps']):
        for i in range(c['count']):
            for j, what in enumerate('pmv'):
                name = '%s/step%d/tensor%d(%d)/%s' % (c['name'], s + 1, i, sizes[i], what)
                same_bits(name + '/twice', got[s][i][j], again[s][i][j])
                if i == c['zero']:
                    same_bits(name + '/zero gradient', got[s][i][j], (p0, m0, v0)[j][i])
                    continue
                # per tensor and per quantity, at its own scale: p ~ scale, m ~ 0.1 .. 1, v ~ 1e-3 .. 1
                check(name, got[s][i][j], w64[s][i][j], w32[s][i][j])


def run_adam_errors(bk):
    """count 0 and 33, NULL pointers, numel 0 (refused today: pinned): GNNPP_ERR_ARG, nothing written."""
    n = 300
    bufs = [Guarded(bk, n) for _ in range(3)]
    gb = bk.put(np.ones(n, np.float32))
    state = Guarded(bk, 8)

    def call(count=2, null=None, numel=n, table=True, st=True):
        tb = AdamTensors()
        for i in range(32):
            tb.p[i], tb.g[i], tb.m[i], tb.v[i], tb.numel[i] = bufs[0].ptr, gb.ptr, bufs[1].ptr, bufs[2].ptr, n
        if null:
            getattr(tb, null)[1] = None
        tb.numel[1] = numel
        tb.count = count
        rc = bk.lib.gnnpp_adam_step(ctypes.byref(tb) if table else None, state.ptr if st else None, LR, 0.9,
                                    0.999, 1e-8, 0.0, 1, bk.stream)
        bk.sync()
        return rc

    table = (('count 0', dict(count=0)), ('count 33', dict(count=33)), ('count -1', dict(count=-1)),
             ('NULL p', dict(null='p')), ('NULL g', dict(null='g')), ('NULL m', dict(null='m')), ('NULL v', dict(null='v')),
             ('NULL table', dict(table=False)), ('NULL state', dict(st=False)), ('numel 0', dict(numel=0)),
             ('numel -5', dict(numel=-5)))
    for name, kw in table:
        assert call(**kw) == ERR_ARG, name
        assert all(b.untouched() for b in bufs) and state.untouched(), name

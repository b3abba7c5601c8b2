"""MAPF cases generated on the device: the step ahead of the expert and of the rollout.

    casegen.generate (this module) -> mapf.distances / mapf.solve / mapf.solve_team -> expert.samples_from_solutions
                                    -> BatchedRollout

The reference draws its cases on the host (offlineExpert/CasesGenerator.py): a random map, a flood fill that leaves one
connected free region (img_fill), start and goal pairs from the free space without duplicates.  gnnpp_casegen
(include/gnnpp_casegen.h, csrc/casegen_kernels.hip) states that generator as a contract on counter hashes -- a case
depends on (seed, case index) alone -- and runs one workgroup per case: the hashed map (or the caller's own), its largest
4-connected free component, N distinct starts and N distinct goals of that component, no agent on its own goal.  Every
agent of a generated case has a path.  There is no CPU fallback.  Positions are (row, col) integers.

The reference's own maps -- CasesGen.mapGen: wall segments grown by random walks on the even lattice, on numpy's legacy
stream -- come from gnnpp_casegen_maze (include/gnnpp_casegen_maze.h, csrc/casegen_maze_kernels.hip), bit for bit what
mapGen draws after np.random.seed(s): maze_maps / enqueue_maze_maps, or generate(..., maps='maze'), which hands them to
the unchanged gnnpp_casegen as the caller's maps.  The closure stays this module's (the largest component), not the
reference's img_fill (a flood from the corner cell); the two agree wherever the corner is free and lies in the largest
free region.
"""
import numpy as np
import torch

from . import _native

MAX_TEAM, MAX_SIDE = _native.ROLLOUT_MAX_TEAM, _native.MAPF_TEAM_MAX_SIDE
OK, TOO_SMALL = _native.CASEGEN_OK, _native.CASEGEN_TOO_SMALL


def threshold_of(density):
    """The obstacle threshold of a density in 0 .. 1: a cell is an obstacle iff its 32-bit hash is below it."""
    return min(int(density * 2 ** 32), 2 ** 32 - 1)


class Cases:
    """Device tensors of one generate call: grid [C,H,W] uint8 (1 = obstacle; the closed map), start, goal [C,N,2] int32
    (row, col), cells [C] int32 (the size of the free region), status [C] int32 (OK, or TOO_SMALL: the region holds
    fewer than max(N, 2) cells, and the case's starts and goals are -1).  grid, start and goal go as they are to
    mapf.distances, mapf.solve, mapf.solve_team and BatchedRollout."""

    def __init__(self, grid, start, goal, cells, status):
        self.grid, self.start, self.goal, self.cells, self.status = grid, start, goal, cells, status

    def __len__(self):
        return int(self.status.shape[0])

    @property
    def ok(self):
        """bool [C] on the device."""
        return self.status == OK

    def yaml(self, c):
        """Case c as the reference's solver input (map dimensions, obstacles, agents with start and goal): the text of
        expert.failure_case_yaml."""
        from . import expert
        if int(self.status[c]) != OK:
            raise _native.GnnppError('case %d is too small: its free region holds %d cells for %d agents'
                                     % (c, int(self.cells[c]), int(self.start.shape[1])))
        return expert.failure_case_yaml(self.grid[c].cpu().numpy(), self.start[c].cpu().numpy(),
                                        self.goal[c].cpu().numpy())


def _check_shape(C, N, H, W):
    C, N, H, W = int(C), int(N), int(H), int(W)
    if C < 1 or not 1 <= N <= MAX_TEAM or C * N > 2 ** 31 - 1:
        raise _native.GnnppError('C >= 1 cases of 1 to %d agents, C * N < 2^31 (got C = %d, N = %d, maps of %d x %d)'
                                 % (MAX_TEAM, C, N, H, W))
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise _native.GnnppError('maps of 1 x 1 to %d x %d cells (got %d x %d, C = %d, N = %d)'
                                 % (MAX_SIDE, MAX_SIDE, H, W, C, N))
    return C, N, H, W


def empty_cases(C, N, H, W, device):
    """The output tensors of enqueue_generate for C cases of N agents on H x W maps."""
    C, N, H, W = _check_shape(C, N, H, W)
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('casegen needs a HIP device (no CPU fallback)')
    return Cases(torch.empty((C, H, W), dtype=torch.uint8, device=dev),
                 torch.empty((C, N, 2), dtype=torch.int32, device=dev), torch.empty((C, N, 2), dtype=torch.int32, device=dev),
                 torch.empty((C,), dtype=torch.int32, device=dev), torch.empty((C,), dtype=torch.int32, device=dev))


def enqueue_generate(out, density=0.1, seed=0, grids=None):
    """gnnpp_casegen alone, on torch's current stream of the tensors' device: one launch, no allocation, no host
    synchronisation, capturable in a HIP graph.  out: from empty_cases; grids: None (hashed maps of `density`) or the
    caller's own raw maps, a contiguous uint8 device tensor [C,H,W] or [H,W] (nonzero = obstacle; `density` is unused)."""
    dev = _native.require_gpu(out.grid, out.start, out.goal, out.cells, out.status, grids)
    C, H, W = (int(v) for v in out.grid.shape)
    N = int(out.start.shape[1])
    if grids is not None and (grids.dtype != torch.uint8 or not grids.is_contiguous() or tuple(grids.shape[-2:]) != (H, W)
                              or grids.dim() not in (2, 3) or (grids.dim() == 3 and grids.shape[0] != C)):
        raise _native.GnnppError('grids must be a contiguous uint8 tensor [%d,%d] or [%d,%d,%d] (got %s %s)'
                                 % (H, W, C, H, W, grids.dtype, tuple(grids.shape)))
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_casegen(
            grids.data_ptr() if grids is not None else None, int(grids is not None and grids.dim() == 3),
            threshold_of(density), int(seed) & 0xffffffff, C, N, H, W, out.grid.data_ptr(), out.start.data_ptr(),
            out.goal.data_ptr(), out.cells.data_ptr(), out.status.data_ptr(), _native.stream_ptr(dev)), 'gnnpp_casegen')


def maze_counts(H, W, density, complexity):
    """(walls, steps) of an H x W maze: the reference's own float expressions (mapGen), so the rounding is its own."""
    return int(density * ((int(H) // 2) * (int(W) // 2))), int(complexity * (5 * (int(H) + int(W))))


def _check_maze(H, W, density, complexity):
    if not (3 <= int(H) <= MAX_SIDE and 3 <= int(W) <= MAX_SIDE):
        raise _native.GnnppError('maze maps of 3 x 3 to %d x %d cells (got %d x %d; below 3 the reference itself raises)'
                                 % (MAX_SIDE, MAX_SIDE, H, W))
    if not 0.0 <= float(density) <= 1.0:
        raise _native.GnnppError('density must be in 0 .. 1 (got %r)' % (density,))
    if not 0.0 <= float(complexity) <= 1.0:
        raise _native.GnnppError('complexity must be in 0 .. 1 (got %r)' % (complexity,))


def enqueue_maze_maps(out, density, complexity, seed=0, seeds=None, words=None):
    """gnnpp_casegen_maze alone, on torch's current stream of the tensor's device: one launch, no allocation, no host
    synchronisation, capturable in a HIP graph.  out: contiguous uint8 device tensor [C,H,W], every byte is written (1 =
    wall).  Map c is what the reference's mapGen(width=W, height=H, complexity, density) returns after
    np.random.seed(seed + c mod 2^32), or after np.random.seed(seeds[c]) with seeds, a contiguous device tensor [C] whose
    32-bit elements are read as unsigned (int32 or uint32).  words: None or a contiguous int32 device tensor [C] that
    receives the number of 32-bit words each map took from its stream."""
    dev = _native.require_gpu(out, seeds, words)
    if dev is None or out.dim() != 3 or out.dtype != torch.uint8 or not out.is_contiguous():
        raise _native.GnnppError('out must be a contiguous uint8 device tensor [C,H,W] (no CPU fallback)')
    C, H, W = (int(v) for v in out.shape)
    _check_maze(H, W, density, complexity)
    if C < 1:
        raise _native.GnnppError('C >= 1 maps (got C = %d)' % C)
    for name, t, kinds in (('seeds', seeds, (torch.int32, getattr(torch, 'uint32', torch.int32))),
                           ('words', words, (torch.int32,))):
        if t is not None and (t.dtype not in kinds or not t.is_contiguous() or tuple(t.shape) != (C,)):
            raise _native.GnnppError('%s must be a contiguous 32-bit integer tensor [%d] (got %s %s)'
                                     % (name, C, t.dtype, tuple(t.shape)))
    walls, steps = maze_counts(H, W, float(density), float(complexity))
    with _native.device_guard(dev):
        _native.check(_native.lib().gnnpp_casegen_maze(
            seeds.data_ptr() if seeds is not None else None, int(seed) & 0xffffffff, C, H, W, walls, steps,
            out.data_ptr(), words.data_ptr() if words is not None else None, _native.stream_ptr(dev)),
            'gnnpp_casegen_maze')


def _device_seeds(seeds, C, dev):
    """seeds (any integers in 0 .. 2^32 - 1, host or device) as the int32 device tensor [C] of their low 32 bits."""
    if seeds is None:
        return None
    if torch.is_tensor(seeds) and seeds.is_cuda and seeds.dtype == torch.int32:
        s = seeds
    else:
        a = np.asarray(seeds.cpu() if torch.is_tensor(seeds) else seeds).astype(np.int64)
        if a.size and (a.min() < 0 or a.max() > 2 ** 32 - 1):
            raise _native.GnnppError('seeds must lie in 0 .. 2^32 - 1, as np.random.seed takes them')
        s = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev)
    if tuple(s.shape) != (int(C),):
        raise _native.GnnppError('seeds must hold one seed per map, [%d] (got %s)' % (C, tuple(s.shape)))
    return s.contiguous()


def maze_maps(C, H, W, device, density=0.1, complexity=0.01, seed=0, seeds=None):
    """C maps of H x W cells as the reference draws them (CasesGen.mapGen), uint8 [C,H,W] on the device, 1 = wall: map c
    from np.random.seed(seed + c mod 2^32), or from seeds[c].  Raw mazes: not closed, see generate(maps='maze')."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _native.GnnppError('casegen needs a HIP device (no CPU fallback)')
    _check_maze(H, W, density, complexity)
    if int(C) < 1:
        raise _native.GnnppError('C >= 1 maps (got C = %d)' % C)
    _native.lib()
    out = torch.empty((int(C), int(H), int(W)), dtype=torch.uint8, device=dev)
    s = _device_seeds(seeds, C, out.device)
    enqueue_maze_maps(out, density, complexity, seed, s)
    out._keep = s                                        # input of the enqueued launch
    return out


def generate(C, N, H, W, device, density=0.1, seed=0, grids=None, maps='uniform', complexity=0.01):
    """C cases of N agents on H x W maps: hashed maps with obstacle density `density`, or, with grids ([C,H,W] or
    [H,W], host or device, nonzero = obstacle), cases drawn on the caller's own maps, or, with maps='maze', on the
    reference's own mazes of (density, complexity), map c from np.random.seed(seed + c mod 2^32) (maze_maps).  Every map
    is closed to its largest 4-connected free component; a case whose component holds fewer than max(N, 2) cells is
    reported in .status (TOO_SMALL), never raised.  The same (seed, arguments) give the same bytes.  Returns Cases."""
    if maps not in ('uniform', 'maze'):
        raise _native.GnnppError("maps must be 'uniform' or 'maze' (got %r)" % (maps,))
    if maps == 'maze':
        if grids is not None:
            raise _native.GnnppError("grids= and maps='maze' are two sources of the raw map: pass one of them")
        _check_shape(C, N, H, W)
        _check_maze(H, W, density, complexity)
    out = empty_cases(C, N, H, W, device)
    if not 0.0 <= float(density) <= 1.0:
        raise _native.GnnppError('density must be in 0 .. 1 (got %r)' % (density,))
    if maps == 'maze':
        _native.lib()
        raw = torch.empty_like(out.grid)
        enqueue_maze_maps(raw, density, complexity, seed)
        enqueue_generate(out, density, seed, raw)
        out._keep = raw                                  # input of the enqueued launch
        out.raw = raw                                    # the maze before the closure
        return out
    if grids is not None:
        g = grids if torch.is_tensor(grids) else torch.as_tensor(np.asarray(grids))
        if g.dim() not in (2, 3) or tuple(g.shape[-2:]) != (int(H), int(W)) or (g.dim() == 3 and g.shape[0] != int(C)):
            raise _native.GnnppError('grids must be [H,W] or [C,H,W] = [%d,%d,%d] (got %s)' % (C, H, W, tuple(g.shape)))
        grids = (g != 0).to(torch.uint8).contiguous().to(out.grid.device)
    _native.lib()
    enqueue_generate(out, density, seed, grids)
    out._keep = grids                                    # input of the enqueued launch
    return out

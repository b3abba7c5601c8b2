"""The shared case table of the maze-map generator (gnnpp_casegen_maze, include/gnnpp_casegen_maze.h): run under the host
emulation (tests/test_emu_casegen_maze.py) and on the device (tests/test_gpu_casegen_maze_cases.py).

The yardstick is tests/golden/maze_maps.npz: maps drawn by the reference's own CasesGen.mapGen after np.random.seed(s), and
the number of 32-bit words numpy's generator gave out for each (tools/gen_maze_golden.py writes it from TABLE below; it is
the only program that needs the reference).  maze_map() is this repository's own plain restatement of the same walk on its
own MT19937; the fixture pins it first (test_the_restatement_equals_the_fixture), and it is the yardstick only where the
fixture has no entry (other seeds, other shapes).  Its two `mutant` switches are wrong on purpose: the tests show that
named cases of the table can tell them.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'maze_maps.npz')
POISON = 0x5a

# name -> dict(C, H, W, density, complexity, seed0 | seeds); a case with `seeds` passes them as an array, the others
# pass seed0 and draw case c from seed0 + c mod 2^32
TABLE = {
    # W // 2 == 1: no word for a coordinate, and every neighbour list has two entries: no word at all
    'side_3x3': dict(C=3, H=3, W=3, density=1.0, complexity=0.2, seed0=0),
    # W // 2 == 2: one-bit coordinates; lists of two entries only
    'side_4x4': dict(C=5, H=4, W=4, density=1.0, complexity=0.1, seed0=1),
    'side_3_by_4': dict(C=2, H=3, W=4, density=1.0, complexity=0.3, seed0=5),
    # odd, not square: x is drawn before y, edge cells with three neighbours
    'odd_5x7': dict(C=6, H=5, W=7, density=0.5, complexity=0.1, seed0=0),
    'odd_21x13': dict(C=4, H=21, W=13, density=0.1, complexity=0.01, seed0=1337),
    # the reference's own setting; six cases are one workgroup and a half
    'reference_20x20': dict(C=6, H=20, W=20, density=0.1, complexity=0.01, seed0=1337),
    # 640 to 710 words: a second refill of the block
    'second_refill_21x13': dict(C=3, H=21, W=13, density=0.5, complexity=0.1, seed0=0),
    # about 2 500 words: four refills or more
    'many_refills_64x48': dict(C=2, H=64, W=48, density=0.2, complexity=0.02, seed0=1337),
    # rows of more than one 64-bit word
    'wide_5x70': dict(C=3, H=5, W=70, density=0.5, complexity=0.05, seed0=3),
    'tall_70x5': dict(C=3, H=70, W=5, density=0.5, complexity=0.05, seed0=3),
    # the side limit
    'limit_256x256': dict(C=1, H=256, W=256, density=0.1, complexity=0.01, seed0=1337),
    'limit_3x256': dict(C=2, H=3, W=256, density=0.5, complexity=0.02, seed0=9),
    # walls == 0: an all-free map; steps == 0: dots only
    'no_walls_20x20': dict(C=2, H=20, W=20, density=0.0, complexity=0.01, seed0=0),
    'no_steps_20x20': dict(C=2, H=20, W=20, density=0.3, complexity=0.0, seed0=0),
    # seed edges: 2^32 - 1, then the wrap to 0
    'seed_wraps_to_zero': dict(C=2, H=20, W=20, density=0.1, complexity=0.01, seed0=2 ** 32 - 1),
    # the seeds as an array, in no order
    'explicit_seeds': dict(C=5, H=10, W=12, density=0.3, complexity=0.05, seeds=[1337, 0, 2 ** 32 - 1, 7, 1]),
}
NAMES = sorted(TABLE)


def counts_of(H, W, density, complexity):
    """(walls, steps) of a map: the reference's own float expressions, so the rounding is the reference's."""
    return int(density * ((H // 2) * (W // 2))), int(complexity * (5 * (H + W)))


def seeds_of(case):
    if 'seeds' in case:
        return np.asarray(case['seeds'], dtype=np.uint32)
    return ((case['seed0'] + np.arange(case['C'], dtype=np.uint64)) % 2 ** 32).astype(np.uint32)


_golden = None


def golden(name):
    """(maps [C,H,W] uint8, words [C] int32, seeds [C] uint32) of a case as the reference made them."""
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    case = TABLE[name]
    params = _golden[name + '/params']
    assert params.tolist() == [case['C'], case['H'], case['W'], *counts_of(case['H'], case['W'], case['density'],
                                                                           case['complexity'])], (name, params)
    assert np.array_equal(_golden[name + '/seeds'], seeds_of(case)), name
    return _golden[name + '/maps'], _golden[name + '/words'], _golden[name + '/seeds']


# ---- the restatement: MT19937 as np.random.seed(s) leaves it, randint's masked rejection on 32-bit words, the walk ------
class Stream:
    """numpy's legacy stream: init_genrand(seed), the standard twist and tempering; .words counts the words given out."""

    def __init__(self, seed):
        mt = [int(seed) & 0xffffffff]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xffffffff)
        self.mt, self.pos, self.words = mt, 624, 0

    def word(self):
        mt = self.mt
        if self.pos == 624:
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7fffffff)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
            self.pos = 0
        y = mt[self.pos]
        self.pos += 1
        self.words += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        return y ^ (y >> 18)

    def randint(self, high):
        """np.random.randint(0, high), high > 0 exclusive: no word when only 0 can come out."""
        rng = high - 1
        if rng == 0:
            return 0
        mask = rng
        for s in (1, 2, 4, 8, 16):
            mask |= mask >> s
        while True:
            v = self.word() & mask
            if v <= rng:
                return v


def maze_map(H, W, walls, steps, seed, mutant=None):
    """-> (map [H,W] uint8, words).  mutant: None | 'inclusive_high' (the pick may take the last neighbour) |
    'y_before_x' (the row is drawn first)."""
    rs = Stream(seed)
    maze = np.zeros((H, W), np.uint8)
    for _ in range(walls):
        if mutant == 'y_before_x':
            y = rs.randint(H // 2) * 2
            x = rs.randint(W // 2) * 2
        else:
            x = rs.randint(W // 2) * 2
            y = rs.randint(H // 2) * 2
        maze[y, x] = 1
        for _ in range(steps):
            nb = []
            if x > 1:
                nb.append((y, x - 2))
            if x < W - 2:
                nb.append((y, x + 2))
            if y > 1:
                nb.append((y - 2, x))
            if y < H - 2:
                nb.append((y + 2, x))
            y_, x_ = nb[rs.randint(len(nb) if mutant == 'inclusive_high' else len(nb) - 1)]
            if maze[y_, x_] == 0:
                maze[y_, x_] = 1
                maze[y_ + (y - y_) // 2, x_ + (x - x_) // 2] = 1
                x, y = x_, y_
    return maze, rs.words


def restate(case, mutant=None):
    """(maps, words) of a table case (or any dict of its form) by maze_map."""
    walls, steps = counts_of(case['H'], case['W'], case['density'], case['complexity'])
    out = [maze_map(case['H'], case['W'], walls, steps, int(s), mutant) for s in seeds_of(case)]
    return np.stack([m for m, _ in out]), np.asarray([w for _, w in out], dtype=np.int32)


def assert_equal_to_golden(name, maps, words):
    want_maps, want_words, _ = golden(name)
    assert maps.dtype == np.uint8 and maps.shape == want_maps.shape, (name, maps.dtype, maps.shape)
    bad = np.argwhere(maps != want_maps)
    assert bad.size == 0, (name, 'first differing (case, row, col):', bad[0].tolist(), len(bad))
    assert np.array_equal(np.asarray(words), want_words), (name, np.asarray(words).tolist(), want_words.tolist())

#!/usr/bin/env python3
"""Write tests/golden/maze_maps.npz: the maps of tests/casegen_maze_cases.TABLE as the REFERENCE draws them.

    python tools/gen_maze_golden.py --reference <checkout of the reference>

CPU only; the one program of this repository that needs the reference.  It imports offlineExpert/CasesGenerator.py and
calls the unbound CasesGen.mapGen(None, width, height, complexity, density) after np.random.seed(s), once per case seed.
That module imports cv2 (used by img_fill only; a stub module stands in when it is missing), parses the command line and
changes the process's CPU affinity at import, so it gets a clean sys.argv and this script runs as a process of its own.

Per table case the file holds  <name>/params = [C, H, W, walls, steps],  <name>/seeds [C] uint32,  <name>/maps [C,H,W]
uint8 and  <name>/words [C] int32: the 32-bit words numpy's MT19937 gave out during the call.  The count is read off
numpy's own state, not off a restatement: after the call the state is (key, pos); a fresh RandomState(s) that has given
out n = 624 * (r - 1) + pos words (r = 0, 1, 2, ... refills) is compared with it until both agree.
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def words_drawn(seed, state):
    _, key, pos = state[:3]
    for r in range(0, 4096):
        n = 624 * (r - 1) + pos
        if n < 0:
            continue
        fresh = np.random.RandomState(seed)
        if n:
            fresh.randint(0, 2 ** 32, size=n, dtype=np.uint32)           # one word per value
        _, fkey, fpos = fresh.get_state()[:3]
        if fpos == pos and np.array_equal(fkey, key):
            return n
    raise RuntimeError('the state after mapGen is not on the stream of seed %d' % seed)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'maze_maps.npz'))
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules['cv2'] = types.ModuleType('cv2')
    sys.path.insert(0, os.path.join(args.reference, 'offlineExpert'))
    import CasesGenerator
    import casegen_maze_cases as mz

    out = {}
    for name in mz.NAMES:
        case = mz.TABLE[name]
        H, W = case['H'], case['W']
        seeds = mz.seeds_of(case)
        maps, words = [], []
        for s in seeds:
            np.random.seed(int(s))
            m = CasesGenerator.CasesGen.mapGen(None, width=W, height=H, complexity=case['complexity'],
                                               density=case['density'])
            words.append(words_drawn(int(s), np.random.get_state()))
            assert m.shape == (H, W) and set(np.unique(m).tolist()) <= {0, 1}
            maps.append(m.astype(np.uint8))
        out[name + '/params'] = np.asarray([case['C'], H, W, *mz.counts_of(H, W, case['density'], case['complexity'])],
                                           dtype=np.int64)
        out[name + '/seeds'] = seeds
        out[name + '/maps'] = np.stack(maps)
        out[name + '/words'] = np.asarray(words, dtype=np.int32)
        print('%-22s C=%d %3dx%-3d walls=%-5d steps=%-3d words=%s' % (name, case['C'], H, W, *out[name + '/params'][3:],
                                                                       words))
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()

"""Write tests/golden/det_step_parent.npz: one deterministic fp32 TD step per shape of tests/det_step_case.py, as THIS build computes it on
the GPU it runs on.

    python tools/gen_det_step_golden.py [--out tests/golden/det_step_parent.npz]

The fixture pins a build: it is recorded from the commit in front of a change that must not move a bit of the deterministic step (the
scheduling of the fixed-order sums), and tests/test_gpu_det_forms.py then holds every later build to it.  Arrays only.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'spatial-intention-maps_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import det_step_case as case                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'det_step_parent.npz'))
    args = ap.parse_args()
    out = {}
    for cin, cout, batch in case.SHAPES:
        first, again = case.run(cin, cout, batch), case.run(cin, cout, batch)
        for k, v in first.items():
            assert np.array_equal(v, again[k]), 'the step does not repeat: %s of %s' % (k, case.key(cin, cout, batch))
            out['%s.%s' % (case.key(cin, cout, batch), k)] = v
        print(case.key(cin, cout, batch), 'loss %.9g td_error %.9g' % (first['loss'], first['td_error']),
              'grad sha256', bytes(first['grad_sha256']).hex()[:16])
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()

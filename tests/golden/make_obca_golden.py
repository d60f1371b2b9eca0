"""
Generates obca_halfplanes_golden.npz by RUNNING THE REFERENCE's own rotation_translation (common/utils.py:412-431, numpy
branch) in the build container -- it reads /root/reference, which never travels.  The function's body is extracted at run
time (make_golden.extract_functions: compiled unmodified from the reference file); only arrays are written, no reference source
is copied.

  poses [n,3]  x, y, heading of a rectangle (the reference's vehicle: length 4.47, width 2.0, mpc.py:105-106);
  A [n,4,2], b [n,4]  its half-plane form {z : A z <= b} as the reference returns it (b squeezed from [4,1]).

The poses cover what the 'obca' constraints see (mpc.py:211-221): headings over several turns, the axis-aligned ones exactly,
centres across the intersection.  tests/test_box_host.py holds tests/box_collision_restated.py halfplanes() to these arrays.

    python tests/golden/make_obca_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, extract_functions      # noqa: E402

LENGTH, WIDTH = 4.47, 2.0


def poses(n=100, seed=5):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, 0] = rng.uniform(-10.0, 60.0, n)
    p[:, 1] = rng.uniform(-30.0, 30.0, n)
    p[:, 2] = rng.uniform(-3.0 * np.pi, 3.0 * np.pi, n)
    p[:8, 2] = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 2 * np.pi, 1e-9, -1e-9]
    p[8] = [0.0, 0.0, 0.0]
    return p


def main():
    if not os.path.isdir(REF):
        raise SystemExit('reference not mounted; fixtures can only be regenerated in the build container')
    fn = extract_functions(os.path.join(REF, 'common', 'utils.py'), ['rotation_translation'], namespace={'np': np})['rotation_translation']
    P = poses()
    A = np.empty((len(P), 4, 2))
    b = np.empty((len(P), 4))
    for i, (x, y, th) in enumerate(P):
        Ai, bi = fn([x, y], th, LENGTH, WIDTH, mode='numpy')
        A[i] = Ai
        b[i] = np.asarray(bi).reshape(4)
    out = os.path.join(HERE, 'obca_halfplanes_golden.npz')
    np.savez(out, poses=P, A=A, b=b, length=LENGTH, width=WIDTH)
    print('wrote', out, A.shape, b.shape)


if __name__ == '__main__':
    main()

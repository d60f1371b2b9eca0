"""The rectangle (OBCA) collision verdict of igt_solve_batch_box_f64 / igt_rollout_batch_box_f64 restated in numpy, from the
definition in include/igtmpc.h alone -- broadcast over [B,C,n_obs,N].  Nothing here calls the library.

Ego and obstacles are rectangles of one size (length x width).  Per obstacle o and node k = 1..N, with the ego's centre
p = (x_k, y_k) and heading psi_k, the obstacle's centre q and heading phi, h = (length/2, width/2), rho = |h|:
  1. gate: |p - q|^2 >= (d_box + 1e-6 + 2 rho)^2 is clear;
  2. separating axes: the four depths of the two frames, depth their minimum;
  3. signed gap: -depth where depth > 0, else the smallest distance of one rectangle's vertex to the other rectangle;
  4. g = d_box + 1e-6 - gap, violated where g > feas_tol;
  5. a non-finite obstacle coordinate or heading (|heading| > 1e6 counts) is no constraint.
"""
import numpy as np

LENGTH, WIDTH = 4.47, 2.0          # the reference's vehicle (mpc.py:105-106)
MARGIN = 1e-6                      # mpc.py:221
HEADING_DOMAIN = 1.0e6
SIGNS = np.array([[1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]])


def half_extents(length=LENGTH, width=WIDTH):
    return np.array([0.5 * length, 0.5 * width])


def gate_radius(length=LENGTH, width=WIDTH, d_box=0.0):
    return d_box + MARGIN + 2.0 * np.hypot(0.5 * length, 0.5 * width)


def halfplanes(x, y, heading, length=LENGTH, width=WIDTH):
    """(A[...,4,2], b[...,4]) with {z : A z <= b} the rectangle of centre (x, y) and the given heading -- the rows in the order
    of the reference's rotation_translation (utils.py:412-431): +length axis, +width axis, -length axis, -width axis."""
    x, y, heading = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float), np.asarray(heading, float))
    c, s = np.cos(heading), np.sin(heading)
    R = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)            # [...,2,2]
    Rt = np.swapaxes(R, -1, -2)
    A = np.concatenate([Rt, -Rt], axis=-2)                                     # [...,4,2]
    centre = np.einsum('...ij,...j->...i', Rt, np.stack([x, y], -1))           # R^T (x, y)
    h = half_extents(length, width)
    b = np.concatenate([h + centre, h - centre], axis=-1)
    return A, b


def _to_frame(dx, dy, c, s):
    """R(angle)^T (dx, dy)"""
    return c * dx + s * dy, -s * dx + c * dy


def depths(px, py, psi, qx, qy, phi, length=LENGTH, width=WIDTH):
    """The four separating-axis depths, stacked on a last axis."""
    h0, h1 = half_extents(length, width)
    dx, dy = qx - px, qy - py
    t0, t1 = _to_frame(dx, dy, np.cos(psi), np.sin(psi))
    u0, u1 = _to_frame(-dx, -dy, np.cos(phi), np.sin(phi))
    th = phi - psi
    c, s = np.abs(np.cos(th)), np.abs(np.sin(th))
    e0, e1 = h0 + h0 * c + h1 * s, h1 + h0 * s + h1 * c
    return np.stack([e0 - np.abs(t0), e1 - np.abs(t1), e0 - np.abs(u0), e1 - np.abs(u1)], -1)


def vertex_distance(px, py, psi, qx, qy, phi, length=LENGTH, width=WIDTH):
    """The smallest, over the eight vertices of one rectangle taken in the other's frame, of |max(|v| - h, 0)|."""
    h = half_extents(length, width)
    best = None
    for (ax, ay, aa, bx, by, ba) in ((px, py, psi, qx, qy, phi), (qx, qy, phi, px, py, psi)):
        # the vertices of rectangle b in the frame of rectangle a
        t0, t1 = _to_frame(bx - ax, by - ay, np.cos(aa), np.sin(aa))
        th = ba - aa
        c, s = np.cos(th), np.sin(th)
        for sg in SIGNS:
            vx = t0 + sg[0] * h[0] * c - sg[1] * h[1] * s
            vy = t1 + sg[0] * h[0] * s + sg[1] * h[1] * c
            d = np.hypot(np.maximum(np.abs(vx) - h[0], 0.0), np.maximum(np.abs(vy) - h[1], 0.0))
            best = d if best is None else np.minimum(best, d)
    return best


def signed_gap(px, py, psi, qx, qy, phi, length=LENGTH, width=WIDTH):
    """Steps 2 and 3 for every pair (no gate): minus the penetration depth on overlap, the distance else."""
    px, py, psi, qx, qy, phi = np.broadcast_arrays(*[np.asarray(v, float) for v in (px, py, psi, qx, qy, phi)])
    with np.errstate(invalid='ignore'):
        depth = depths(px, py, psi, qx, qy, phi, length, width).min(-1)
        return np.where(depth > 0.0, -depth, vertex_distance(px, py, psi, qx, qy, phi, length, width))


def edge_distance(px, py, psi, qx, qy, phi, length=LENGTH, width=WIDTH):
    """An independent form of the distance of two rectangles that do not overlap: the smallest distance of a vertex of one to an
    edge (a segment) of the other, over all 2 x 4 x 4 pairs.  Scalar poses."""
    def corners(x, y, a):
        h = half_extents(length, width)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        loop = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]]) * h
        return loop @ R.T + np.array([x, y])
    P, Q = corners(px, py, psi), corners(qx, qy, phi)
    best = np.inf
    for V, E in ((P, Q), (Q, P)):
        for v in V:
            for i in range(4):
                a, b = E[i], E[(i + 1) % 4]
                t = np.clip(np.dot(v - a, b - a) / np.dot(b - a, b - a), 0.0, 1.0)
                best = min(best, float(np.linalg.norm(v - (a + t * (b - a)))))
    return best


def margins(X, pose, length=LENGTH, width=WIDTH, d_box=0.0):
    """g[B,C,n_obs,N] of trajectories X[B,C,7,N+1] (rows 0, 1, 6: x, y, heading) against pose[B,n_obs,3,N+1], nodes 1..N:
    g = d_box + 1e-6 - gap inside the gate, -inf where the pair is clear by the gate or the obstacle's node is no constraint,
    NaN where the ego's pose is not finite (no verdict: the non-finite bit reports it).  Also -> inside[B,C,n_obs,N], gap."""
    X = np.asarray(X, float); pose = np.asarray(pose, float)
    px, py, psi = (X[:, :, i, None, 1:] for i in (0, 1, 6))                    # [B,C,1,N]
    qx, qy, phi = (pose[:, None, :, i, 1:] for i in (0, 1, 2))                 # [B,1,n_obs,N]
    with np.errstate(invalid='ignore', over='ignore'):
        live = np.isfinite(qx) & np.isfinite(qy) & (np.abs(phi) <= HEADING_DOMAIN)
        qx, qy, phi = np.where(live, qx, 0.0), np.where(live, qy, 0.0), np.where(live, phi, 0.0)
        d2 = (px - qx) ** 2 + (py - qy) ** 2
        inside = live & (d2 < gate_radius(length, width, d_box) ** 2)          # a NaN ego position is inside no gate
        gap = signed_gap(px, py, psi, qx, qy, phi, length, width)
        g = np.where(inside, d_box + MARGIN - gap, -np.inf)
    return g, inside, gap


def collides(X, pose, feas_tol=1e-6, **kw):
    """[B,C] the collision verdict (IGT_VIOL_COLLISION) of every trajectory."""
    g = margins(X, pose, **kw)[0]
    with np.errstate(invalid='ignore'):
        return (g > feas_tol).any(axis=(2, 3))

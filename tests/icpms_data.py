"""Inputs for the multi-start ICP tests: planar truths and the cluster centroids that should match them (MainForm.ICP:
centroids (x, y, 0) against the truth list), moved by a planted rigid transform.  All from fixed seeds."""
import numpy as np


def rz(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def angle_of(M):
    """Rotation angle about z of the 3x3 block of M (a reflection diag(1, -1, 1) first undone when det < 0)."""
    R = np.asarray(M)[:3, :3]
    if np.linalg.det(R) < 0:
        R = R @ np.diag([1.0, -1.0, 1.0])
    return np.arctan2(R[1, 0], R[0, 0])


def angle_diff(a, b):
    return abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def planted(truths, theta, seed, keep=0.9, noise=0.0, mirror=False, shift=(37.0, -21.0)):
    """centers = T^-1 (a `keep` subset of the truths) + noise, where T = [Rz(theta) | t] (after diag(1, -1, 1) when
    mirror) is the transform ICP should recover: T(centers) ~ truths."""
    rng = np.random.default_rng(seed)
    sub = truths[np.sort(rng.choice(len(truths), int(round(keep * len(truths))), replace=False))]
    R = rz(theta) @ (np.diag([1.0, -1.0, 1.0]) if mirror else np.eye(3))
    t = np.array([shift[0], shift[1], 0.0])
    cen = (sub - t) @ R  # R^T (p - t), row form
    cen[:, :2] += rng.normal(0.0, noise, (len(cen), 2)) if noise else 0.0
    cen[:, 2] = 0.0
    return np.ascontiguousarray(cen), R, t


def random_truths(n, seed, extent=400.0):
    """n planar points, uniform in [0, extent]^2, z = 0: no lattice, no symmetry."""
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(0.0, extent, (n, 2)), np.zeros(n)]


def l_lattice(nx, ny, step=10.0, cut=0.5):
    """Square lattice of nx x ny points with the top-right (cut x cut) part removed: an L-shaped region, so that no
    lattice symmetry maps the set onto itself."""
    pts = [(i * step, j * step) for j in range(ny) for i in range(nx)
           if not (i >= nx * (1 - cut) and j >= ny * (1 - cut))]
    a = np.array(pts, np.float64)
    return np.c_[a, np.zeros(len(a))]

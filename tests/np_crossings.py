"""The reference of tests/test_crossings.py: art_cast_crossings' semantics in numpy.

(a) which triangles accept a ray is the oracle's answer, one triangle at a time: the rows of test_cast_multi.hit_table.  Nothing of accept() is restated here.
(b) det32      the orientation of a row: det = dot3(e1, cross3(d, e2)) in float32 with the device's operations in the device's order -- np_sweep._fma is exact fmaf --
               on np_closest.world_triangles' e1, e2 (the DevTri fields) and the ray's direction as given
(c) det64      a float64 witness of the same sign that shares none of that code: -d . ((w1 - w0) x (w2 - w0)) from the world VERTICES, numpy's cross and sum
(d) crossings  (entries, exits) a ray: the rows with det32 > 0 and with det32 < 0 (accept() has excluded det == 0)
(e) inside_rays / vote / points_inside: Renderer.points_inside's three rays a point and its majority, restated

Seeds: random_rays(4096, 7) are the rays of test_cast_multi's tables, and the share of rows inside the witness's band is far below the 1 % cap with them (cornell 0 of
6 535 rows, sponza_like(0.05) 0 of 13 019: printed by test_the_reference_is_tied_down); no other seed was needed.  The probe points of the helpers' tests are
numpy.random.default_rng(11).uniform(-1, 1, (8192, 3)): the reference's vote has no miss with them (asserted first in test_the_vote_of_the_reference_is_the_analytic_answer)."""
import numpy as np

from np_sweep import _fma

F = np.float32
# Renderer.INSIDE_DIRECTIONS, written down a second time on purpose: test_crossings compares the two
DIRECTIONS = np.array([[0.57291365, 0.31830987, 0.75487767], [-0.43016213, 0.81649658, 0.38490018], [0.26794919, -0.61803399, -0.73908513]], F)


def _cross3(a, b):
    """art_device.h's cross3 on columns: fmaf(a.y, b.z, -(a.z * b.y)), ..."""
    return [_fma(a[1], b[2], -(a[2] * b[1]), F), _fma(a[2], b[0], -(a[0] * b[2]), F), _fma(a[0], b[1], -(a[1] * b[0]), F)]


def _dot3(a, b):
    """art_device.h's dot3: fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))"""
    return _fma(a[2], b[2], _fma(a[1], b[1], a[0] * b[0], F), F)


def det32(T, rays, gid, ray):
    """det of moller_trumbore for the pairs (ray[k], gid[k]), float32, bit for bit"""
    cols = lambda a: [np.ascontiguousarray(a[:, k], F) for k in range(3)]   # noqa: E731
    d, e1, e2 = cols(np.asarray(rays, F)[ray, 4:7]), cols(T["e1"][gid]), cols(T["e2"][gid])
    with np.errstate(all="ignore"):
        return _dot3(e1, _cross3(d, e2))


def det64(T, rays, gid, ray):
    """-> (det, band): the witness's det in float64 from the world vertices, and 1e-6 * |e1| * |d x e2|, below which the witness does not vouch for a sign"""
    w = np.asarray(T["w"], np.float64)[gid]
    d = np.asarray(rays, np.float64)[ray, 4:7]
    a, b = w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]
    det = -(d * np.cross(a, b)).sum(axis=1)
    band = 1e-6 * np.linalg.norm(a, axis=1) * np.linalg.norm(np.cross(d, b), axis=1)
    return det, band


def crossings(tab, T, rays, keep=None):
    """(n, 2) int32 (entries, exits) from the rows of a hit table (those of `keep`)"""
    n = np.asarray(rays).reshape(-1, 8).shape[0]
    rows = np.arange(tab["ray"].size) if keep is None else np.flatnonzero(keep)
    ray, gid = tab["ray"][rows], tab["gid"][rows]
    det = det32(T, rays, gid, ray)
    assert not (det == 0).any() and not np.isnan(det).any(), "accept() excludes det == 0"
    out = np.zeros((n, 2), np.int32)
    out[:, 0] = np.bincount(ray[det > 0], minlength=n)
    out[:, 1] = np.bincount(ray[det < 0], minlength=n)
    return out


def inside_rays(points):
    """ray 3i + j: from point i along DIRECTIONS[j], tmin 0, tmax inf"""
    p = np.asarray(points, F).reshape(-1, 3)
    rays = np.zeros((p.shape[0], 3, 8), F)
    rays[:, :, 0:3] = p[:, None, :]
    rays[:, :, 4:7] = DIRECTIONS[None]
    rays[:, :, 7] = np.inf
    return rays.reshape(-1, 8)


def vote(cross, rule):
    """the majority of three rays a point: (n,) uint8 from the (3n, 2) counts"""
    c = np.asarray(cross).reshape(-1, 3, 2).astype(np.int64)
    v = ((c[..., 0] + c[..., 1]) & 1) == 1 if rule == "parity" else c[..., 1] > c[..., 0]
    return (v.sum(axis=1) >= 2).astype(np.uint8)

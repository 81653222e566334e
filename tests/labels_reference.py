"""The numpy reference of ls_object_labels (include/lidarshooter_hip.h): the reduction over hit records, restated from the
header's counting rule over float32 points, and the footprint -- per geometry, the rays the existing brute force
(test_gpu_rays._brute: lso_tri_intersect from each ray's origin) finds a hit for in the scene of that geometry alone."""
import numpy as np

INV = 0xFFFFFFFF
LABEL_DTYPE = np.dtype([("n_hits", "<u4"), ("n_alone", "<u4"), ("t_min", "<f4"), ("ray_min", "<u4"), ("t_max", "<f4"), ("ray_max", "<u4"),
                        ("lo", "<f4", 3), ("hi", "<f4", 3), ("flags", "<u4"), ("reserved", "<u4", 3)])


def empty_labels(n_labels):
    out = np.zeros(n_labels, LABEL_DTYPE)
    out["t_min"], out["lo"] = np.inf, np.inf
    out["t_max"], out["hi"] = -np.inf, -np.inf
    out["ray_min"], out["ray_max"] = INV, INV
    return out


def _key(f):
    """float32 -> uint32 of the same order, -0 below +0"""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def rays_walked(rays):
    """bool per ray: one ls_trace_rays walks (finite origin and direction, direction non-zero, tmin <= tmax)"""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return (np.all(np.isfinite(r[:, 0:3]), axis=1) & np.all(np.isfinite(r[:, 4:7]), axis=1) & np.any(r[:, 4:7] != 0, axis=1)
                & (r[:, 3] <= r[:, 7]))


def record_points(records, rays):
    """o + t d per axis in float32, one product and one sum, for records (n, 4) uint32 whose ray index is in range (others: 0)"""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    rec = np.asarray(records, np.uint32).reshape(-1, 4)
    p = np.zeros((rec.shape[0], 3), np.float32)
    ok = rec[:, 0] < r.shape[0]
    t = rec[ok, 3].view(np.float32)
    with np.errstate(all="ignore"):
        prod = (t[:, None] * r[rec[ok, 0], 4:7]).astype(np.float32)
        p[ok] = (r[rec[ok, 0], 0:3] + prod).astype(np.float32)
    return p


def counted(records, geoms, n_labels, ray_bound, rays=None):
    """the header's rule: which records count.  records (n, 4) uint32 (ray, geom, prim, t bits); geoms {geomID: element count} of
    the committed scene; rays: the caller's (n_rays, 8) float32, or None for sensor rays"""
    rec = np.asarray(records, np.uint32).reshape(-1, 4)
    t = rec[:, 3].copy().view(np.float32)
    n_elems = np.zeros(max(n_labels, 1), np.int64)
    for g, ne in geoms.items():
        if g < n_labels:
            n_elems[g] = ne
    with np.errstate(invalid="ignore"):
        ok = (rec[:, 1] < n_labels) & (rec[:, 0] < ray_bound) & np.isfinite(t) & (t >= 0)
    gsafe = np.where(rec[:, 1] < n_labels, rec[:, 1], 0).astype(np.int64)
    present = np.zeros(max(n_labels, 1), bool)
    for g in geoms:
        if g < n_labels:
            present[g] = True
    ok &= present[gsafe] & (rec[:, 2].astype(np.int64) < n_elems[gsafe])
    if rays is not None:
        walked = rays_walked(rays)
        ok &= walked[np.where(rec[:, 0] < ray_bound, rec[:, 0], 0).astype(np.int64)] if walked.shape[0] else False
    return ok


def reduce_records(records, points, geoms, n_labels, ray_bound, rays=None):
    """-> LABEL_DTYPE[n_labels] with n_alone = 0: counts by np.bincount, the rest by plain loops over the geometries.
    points: float32 (n, 3), the records' points (a frame's points32 xyz, or record_points)"""
    rec = np.asarray(records, np.uint32).reshape(-1, 4)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    ok = counted(rec, geoms, n_labels, ray_bound, rays)
    out = empty_labels(n_labels)
    for g in geoms:
        if g < n_labels:
            out["flags"][g] = 1
    out["n_hits"] = np.bincount(rec[ok, 1].astype(np.int64), minlength=n_labels)[:n_labels]
    for g in range(n_labels):
        m = ok & (rec[:, 1] == g)
        if not np.any(m):
            continue
        tb = rec[m, 3] & np.uint32(0x7FFFFFFF)          # t >= 0: its bits order as t does (a -0 counts as +0)
        ray = rec[m, 0]
        out["t_min"][g] = tb.min().view(np.float32)
        out["ray_min"][g] = ray[tb == tb.min()].min()
        out["t_max"][g] = tb.max().view(np.float32)
        out["ray_max"][g] = ray[tb == tb.max()].min()
        k = np.stack([_key(pts[m, a]) for a in range(3)], axis=1)
        out["lo"][g] = _unkey(k.min(axis=0))
        out["hi"][g] = _unkey(k.max(axis=0))
    return out


def footprint(oracle, sensor, ml, rays, n_labels):
    """-> (n_alone int64[n_labels], hit bool[n_rays, n_labels]): column g = the brute force over the scene of geometry g alone
    (assemble_scene keeps the geomID); a geometry whose id is >= n_labels has no column"""
    from test_gpu_rays import _brute
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    M = np.zeros((rays.shape[0], n_labels), bool)
    for entry in ml:
        g = int(entry[0])
        if g < n_labels:
            M[:, g] = _brute(oracle, oracle.assemble_scene(sensor, [entry]), rays)[:, 1] != INV
    return M.sum(axis=0).astype(np.int64), M

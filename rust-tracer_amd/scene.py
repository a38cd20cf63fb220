"""Host-side Scene of the drop-in: what `Scene`, `SphericalGroup::pyramid` and `Scene::default()` are in the
reference (render.rs:138-167, group.rs:27-66), kept as the flat DFS arrays the C ABI consumes.

All scene arithmetic is done in the scene's REAL type with numpy scalars (IEEE, one rounding per operation,
reference operation order) -- centres accumulate rounding level by level, so the builder replays the
recursion instead of using a closed form.  Rendering never happens here; see render.py / capi.py."""
import contextlib
import ctypes as C
import sys

import numpy as np

from . import capi


def _real(precision):
    return np.float32 if precision == capi.RT_F32 else np.float64


def _tmax_array(tmax, R, n, name="tmax"):
    """A query's tmax (or radius: `name`) as a contiguous REAL[n]: one value (a Python float, a 0-d array) is rounded to REAL; an array
    must already be REAL."""
    t = np.asarray(tmax)
    if t.ndim == 0 and t.dtype.kind in "fiu":
        t = t.astype(R)
    if t.dtype != R or t.size not in (1, n):
        raise ValueError("%s must be one value or an (n,) array of %s" % (name, np.dtype(R).name))
    return np.ascontiguousarray(np.broadcast_to(t.reshape(-1), (n,)))


def _rows_text(cols, rows, optional):
    return ("None or " if optional else "") + ("a non-empty (n, %d)" % cols if rows is None else "a (%d, %d)" % (rows, cols))


_N, _ITEMS = object(), object()              # _list_query: an input with as many rows as there are queries / as the scene has items
_NO_STREAM = contextlib.nullcontext(())      # the host side's scope: a host entry takes no stream and returns when it is done


class _HostSide:
    """A call's arguments and results as numpy arrays, for a scene of REAL `R`: what the host entries take.  The checks raise ValueError
    and hand back what the entry can read: contiguous arrays.  _DeviceSide has the same methods; a dtype is named "R", np.int32,
    np.uint32 or np.uint64 on both sides."""
    suffix, trims = "", True

    def __init__(self, R):
        self.R, self.real = R, np.dtype(R).name
        self.types = {"R": R, np.int32: np.int32, np.uint32: np.uint32, np.uint64: np.uint64}

    def scope(self, scene, stream, tensors):
        return _NO_STREAM

    def real_rows(self, x, name, cols, rows=None, optional=False):
        """x: (n, cols) of REAL -- n > 0, or n = rows; None passes where optional."""
        if x is None and optional:
            return None
        if not isinstance(x, np.ndarray) or x.dtype != self.R or x.ndim != 2 or x.shape[1] != cols or x.shape[0] == 0 or (rows is not None and x.shape[0] != rows):
            raise ValueError("%s must be %s numpy array of %s (or a torch tensor on the scene's device)" % (name, _rows_text(cols, rows, optional), self.real))
        return np.ascontiguousarray(x)

    def per_query(self, x, name, n):
        """x: None, one value (rounded to REAL) or (n,) of REAL -> REAL[n]."""
        return None if x is None else _tmax_array(x, self.R, n, name)

    def exclude(self, x, n):
        if x is None:
            return None
        ex = np.asarray(x)
        if ex.dtype != np.int32 or ex.shape != (n,):
            raise ValueError("exclude must be None or an (n,) int32 array")
        return np.ascontiguousarray(ex)

    def order(self, x, n):
        """An index array: contiguous uint32[n] (whether it is a permutation is the library's check)."""
        o = np.asarray(x)
        if o.dtype.kind not in "iu" or o.shape != (n,):
            raise ValueError("order must be None, True or an (n,) integer array")
        if o.dtype != np.uint32 and n and (int(o.min()) < 0 or int(o.max()) > 0xFFFFFFFF):      # (the cast below would wrap it into range)
            raise ValueError("order holds an index outside 0 .. 2^32 - 1")
        return np.ascontiguousarray(o, dtype=np.uint32)

    def empty(self, shape, dt):
        return np.empty(shape, dtype=self.types[dt])

    def copy(self, x):
        return x.copy()

    def check_out(self, out, specs):
        res = tuple(out)
        if len(res) != len(specs) or any(not isinstance(a, np.ndarray) or a.dtype != self.types[dt] or a.shape != shape or not a.flags.c_contiguous
                                         for a, (shape, dt) in zip(res, specs)):
            raise ValueError("out: contiguous arrays of " + ", ".join("%s %s" % (np.dtype(self.types[dt]).name, shape) for shape, dt in specs))
        return res

    @staticmethod
    def ptr(x):
        if x is None:
            return None
        try:
            return C.addressof(C.c_char.from_buffer(x))                          # a third of the time x.ctypes.data takes
        except (TypeError, ValueError):                                          # (a read-only or an empty array)
            return x.ctypes.data

    @staticmethod
    def total_cell():
        """(where a list entry writes its total, the pointer to it)."""
        total = C.c_uint64(0)
        return total, C.byref(total)

    @staticmethod
    def read_total(total):
        return int(total.value)


class _DeviceSide:
    """A call's arguments and results as torch tensors on one device, for a scene of REAL `R`: what the _device entries take.  Made once
    per (precision, device); use it inside its scope, where what it allocates belongs to the call's stream.  Offsets and totals are
    int64 here: the same bits as the host side's uint64."""
    suffix, trims = "_device", False

    def __init__(self, torch, R, device):
        self.torch, self.R, self.dev = torch, R, torch.device("cuda", device)
        self.real = torch.float32 if R == np.float32 else torch.float64
        self.types = {"R": self.real, np.int32: torch.int32, np.uint32: torch.uint32, np.uint64: torch.int64}

    def scope(self, scene, stream, tensors):
        return scene._stream_scope(self.torch, stream, tensors)

    def real_rows(self, x, name, cols, rows=None, optional=False):
        if x is None and optional:
            return None
        if not isinstance(x, self.torch.Tensor) or x.dtype != self.real or x.dim() != 2 or x.shape[1] != cols or x.shape[0] == 0 or x.device != self.dev \
                or (rows is not None and x.shape[0] != rows):
            raise ValueError("%s must be %s %s tensor on %s" % (name, _rows_text(cols, rows, optional), self.real, self.dev))
        return x.contiguous()

    def per_query(self, x, name, n):
        if x is None:
            return None
        if not isinstance(x, self.torch.Tensor):
            return self.torch.from_numpy(_tmax_array(x, self.R, n, name).copy()).to(self.dev)     # (a broadcast view is read-only)
        if x.dim() == 0 and x.dtype.is_floating_point:
            x = x.to(self.real)                                              # one value: rounded to the scene's REAL
        if x.dtype != self.real or x.numel() not in (1, n):
            raise ValueError("%s must be a %s value or (n,) tensor" % (name, self.real))
        return x.to(self.dev).reshape(-1).expand(n).contiguous()

    def exclude(self, x, n):
        if x is None:
            return None
        if not isinstance(x, self.torch.Tensor) or x.dtype != self.torch.int32 or x.shape != (n,) or x.device != self.dev:
            raise ValueError("exclude must be None or an (n,) int32 tensor on %s" % self.dev)
        return x.contiguous()

    def order(self, x, n):
        """An index tensor: contiguous uint32 / int32 [n] on the scene's device."""
        if not isinstance(x, self.torch.Tensor) or x.dtype not in (self.torch.uint32, self.torch.int32) or x.shape != (n,) or x.device != self.dev:
            raise ValueError("order must be None, True or an (n,) uint32 / int32 tensor on %s" % self.dev)
        return x.contiguous()

    def empty(self, shape, dt):
        return self.torch.empty(shape, dtype=self.types[dt], device=self.dev)

    def copy(self, x):
        return x.clone()

    def check_out(self, out, specs):
        res = tuple(out)
        specs = [(shape, self.types[dt]) for shape, dt in specs]
        if len(res) != len(specs) or any(not isinstance(a, self.torch.Tensor) or a.dtype != dt or tuple(a.shape) != shape or a.device != self.dev or not a.is_contiguous()
                                         for a, (shape, dt) in zip(res, specs)):
            raise ValueError("out: contiguous tensors on %s of %s" % (self.dev, ", ".join("%s %s" % (dt, shape) for shape, dt in specs)))
        return res

    @staticmethod
    def ptr(x):
        return None if x is None else x.data_ptr()

    def total_cell(self):
        total = self.torch.zeros((), dtype=self.torch.int64, device=self.dev)
        return total, total.data_ptr()

    @staticmethod
    def read_total(total):
        return int(total.item())


_HOST_SIDES = {capi.RT_F32: _HostSide(np.float32), capi.RT_F64: _HostSide(np.float64)}
_DEVICE_SIDES = {}                           # (precision, device) -> _DeviceSide, made on first use


def ray_keys(rays):
    """The 32-bit sort key rt_ray_order gives each ray of `rays` (n x 6: pos.xyz, dir.xyz; float32 or float64) -> uint32[n], restated in numpy
    operation for operation (include/rtrace_hip.h states it): rt_ray_order's order is np.argsort(ray_keys(rays), kind="stable").  High 9
    bits: the Morton code of the origin's cell in the batch's own origin box (8 cells per axis; all 0 for a batch with one origin); then 3
    bits for the direction's dominant axis and its sign; low 20 bits: the Morton code of the two other direction components, 10 bits each."""
    r = np.asarray(rays)
    if r.ndim != 2 or r.shape[1] != 6 or r.shape[0] == 0 or r.dtype not in (np.float32, np.float64):
        raise ValueError("rays must be a non-empty (n, 6) array of float32 or float64")
    r = r.astype(np.float64)                                             # exact
    pos, d = r[:, :3], r[:, 3:]
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = np.float64((hi - lo).max())
    scale = np.float64(0.0)
    if ext > 0.0:
        e = max((int(ext.view(np.uint64)) >> 52 & 0x7FF) - 1022, -1000)   # ext < 2^e
        scale = np.ldexp(np.float64(1.0), 3 - e)
    c = np.minimum(np.maximum((pos - lo) * scale, 0.0), 7.0).astype(np.uint32)
    axis = np.argmax(np.abs(d), axis=1)                                  # the first of equal maxima
    rows = np.arange(len(d))
    sign = (d[rows, axis] < 0.0).astype(np.uint32)
    q = [np.minimum(np.maximum((d[rows, (axis + 1 + b) % 3] + 1.0) * 512.0, 0.0), 1023.0).astype(np.uint32) for b in (0, 1)]
    m3 = np.zeros(len(d), dtype=np.uint32)
    for i in range(3):
        for a in range(3):
            m3 |= ((c[:, a] >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + a)
    m2 = np.zeros(len(d), dtype=np.uint32)
    for i in range(10):
        for b in range(2):
            m2 |= ((q[b] >> np.uint32(i)) & np.uint32(1)) << np.uint32(2 * i + b)
    return (m3 << np.uint32(23)) | ((np.uint32(2) * axis.astype(np.uint32) + sign) << np.uint32(20)) | m2


def sphere_keys(spheres):
    """The 30-bit sort key rt_sphere_order gives each sphere of `spheres` (n x 4: cx, cy, cz, r; float32 or float64) -> uint32[n], restated in
    numpy operation for operation (include/rtrace_hip.h states it): the sphere order, and the order rt_scene_rebuild puts the spheres in, is
    np.argsort(sphere_keys(spheres), kind="stable").  The Morton code of the centre's cell in the batch's own centre box, 1024 cells per
    axis; the radii take no part, and a batch whose centres are all the same has every key 0."""
    s = np.asarray(spheres)
    if s.ndim != 2 or s.shape[1] != 4 or s.shape[0] == 0 or s.dtype not in (np.float32, np.float64):
        raise ValueError("spheres must be a non-empty (n, 4) array of float32 or float64")
    c = s[:, :3].astype(np.float64)                                      # exact
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = np.float64((hi - lo).max())
    scale = np.float64(0.0)
    if ext > 0.0:
        e = max((int(ext.view(np.uint64)) >> 52 & 0x7FF) - 1022, -1000)   # ext < 2^e
        scale = np.ldexp(np.float64(1.0), 10 - e)
    q = np.minimum(np.maximum((c - lo) * scale, 0.0), 1023.0).astype(np.uint32)
    key = np.zeros(len(c), dtype=np.uint32)
    for i in range(10):
        for a in range(3):
            key |= ((q[:, a] >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + a)
    return key


def sphere_gaps(points, spheres):
    """The surface gap between every point of `points` (n x 3) and every sphere of `spheres` (m x 4: cx, cy, cz, r) -> REAL[n, m], the metric
    of rt_near_spheres restated in numpy bit for bit (include/rtrace_hip.h states it), in the arrays' dtype (float32 or float64, the same for
    both), every operation rounded once:  rr = r * r;  v = c - p;  vv = (v.x*v.x + v.y*v.y) + v.z*v.z;  gap = sqrt(vv) - sqrt(rr) where
    rr > 0, else +inf.  Negative inside the sphere.  A record without a positive rr -- radius 0: a dead slot, a dead group's bound -- is at
    +inf from every point.  DeviceScene.near lists, per point, the k smallest of a row (ties by index) or counts those below a radius."""
    p, s = np.asarray(points), np.asarray(spheres)
    if p.dtype not in (np.float32, np.float64) or s.dtype != p.dtype or p.ndim != 2 or p.shape[1] != 3 or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("points must be (n, 3) and spheres (m, 4), both float32 or both float64")
    R = p.dtype.type
    rr = s[:, 3] * s[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = s[None, :, :3] - p[:, None, :]
        vv = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        gap = np.sqrt(vv) - np.sqrt(np.where(rr > 0, rr, R(1.0)))[None, :]
    return np.where((rr > 0)[None, :], gap, R(np.inf)).astype(R, copy=False)


def pair_gaps(spheres, i, j):
    """The gap of the pairs (i[k], j[k]) of `spheres` (m x 4: cx, cy, cz, r) -> REAL[len(i)], the metric of rt_scene_contacts restated in
    numpy bit for bit (include/rtrace_hip.h states it), in the array's dtype (float32 or float64), every operation rounded once:
    rr = r * r;  v = c_j - c_i;  vv = (v.x*v.x + v.y*v.y) + v.z*v.z;  gap = (sqrt(vv) - sqrt(rr_j)) - sqrt(rr_i) where rr_i > 0 and
    rr_j > 0, else +inf: sphere_gaps of sphere j from the centre of sphere i, minus the radius of sphere i.  The library always takes the
    lower slot as i.  A record without a positive rr -- radius 0: a dead slot -- is at +inf from every sphere, in either place.
    DeviceScene.contacts lists the pairs i < j with !(gap >= margin)."""
    s = np.asarray(spheres)
    if s.dtype not in (np.float32, np.float64) or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("spheres must be an (m, 4) array of float32 or float64")
    i, j = np.asarray(i), np.asarray(j)
    if i.dtype.kind not in "iu" or j.dtype.kind not in "iu" or i.ndim != 1 or i.shape != j.shape:
        raise ValueError("i and j must be integer arrays of one shape, (k,)")
    if i.size and (min(int(i.min()), int(j.min())) < 0 or max(int(i.max()), int(j.max())) >= s.shape[0]):
        raise ValueError("i and j must be rows of spheres")
    R = s.dtype.type
    rr = s[:, 3] * s[:, 3]
    rri, rrj = rr[i], rr[j]
    solid = (rri > 0) & (rrj > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        v = s[j, :3] - s[i, :3]
        vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        gap = (np.sqrt(vv) - np.sqrt(np.where(rrj > 0, rrj, R(1.0)))) - np.sqrt(np.where(rri > 0, rri, R(1.0)))
    return np.where(solid, gap, R(np.inf)).astype(R, copy=False)


def overlap_gaps(queries, spheres):
    """The gap between every query sphere of `queries` (n x 4: px, py, pz, q) and every sphere of `spheres` (m x 4: cx, cy, cz, r) ->
    REAL[n, m], the metric of rt_overlap_spheres restated in numpy bit for bit (include/rtrace_hip.h states it), in the arrays' dtype
    (float32 or float64, the same for both), every operation rounded once:  rr = r * r;  v = c - p;  vv = (v.x*v.x + v.y*v.y) + v.z*v.z;
    gap = (sqrt(vv) - sqrt(rr)) - q where rr > 0, else +inf: sphere_gaps from the query's centre, minus the query's radius.  With q = 0 it
    is sphere_gaps; with a scene's own spheres as the queries and q = sqrt(r * r) it is pair_gaps.  A record without a positive rr --
    radius 0: a dead slot -- is at +inf from every query.  DeviceScene.overlaps lists, per query with q >= 0, the spheres with
    !(gap >= margin); a query whose q is not >= 0 carries no query there, and its row here is whatever the arithmetic gives."""
    qs, s = np.asarray(queries), np.asarray(spheres)
    if qs.dtype not in (np.float32, np.float64) or s.dtype != qs.dtype or qs.ndim != 2 or qs.shape[1] != 4 or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("queries must be (n, 4) and spheres (m, 4), both float32 or both float64")
    R = qs.dtype.type
    rr = s[:, 3] * s[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = s[None, :, :3] - qs[:, None, :3]
        vv = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        gap = (np.sqrt(vv) - np.sqrt(np.where(rr > 0, rr, R(1.0)))[None, :]) - qs[:, 3][:, None]
    return np.where((rr > 0)[None, :], gap, R(np.inf)).astype(R, copy=False)


def box_gaps(boxes, spheres):
    """The gap between every axis-aligned box of `boxes` (n x 6: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z) and every sphere of `spheres` (m x 4:
    cx, cy, cz, r) -> REAL[n, m], the metric of rt_overlap_boxes restated in numpy bit for bit (include/rtrace_hip.h states it), in the
    arrays' dtype (float32 or float64, the same for both), every operation rounded once:  rr = r * r;  per axis e = lo - c, f = c - hi,
    e = f where f > e, e = 0 where not e > 0;  dd = (e.x*e.x + e.y*e.y) + e.z*e.z;  gap = sqrt(dd) - sqrt(rr) where rr > 0, else +inf.
    The distance from the box to the sphere's surface, floored at -r: a centre inside the box has gap = -r, however deep it lies.  A
    point box lo == hi == p gives overlap_gaps with q = 0.  Infinite sides are slabs and half-spaces; the all-infinite box is at
    -sqrt(rr) from every live sphere.  A record without a positive rr -- radius 0: a dead slot -- is at +inf from every box.
    DeviceScene.box_overlaps lists, per box with lo <= hi on every axis, the spheres with !(gap >= margin); a box that is inverted or
    holds a NaN carries no query there, and its row here is whatever the arithmetic gives."""
    b, s = np.asarray(boxes), np.asarray(spheres)
    if b.dtype not in (np.float32, np.float64) or s.dtype != b.dtype or b.ndim != 2 or b.shape[1] != 6 or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("boxes must be (n, 6) and spheres (m, 4), both float32 or both float64")
    R = b.dtype.type
    rr = s[:, 3] * s[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        c = s[None, :, :3]
        e = b[:, None, :3] - c
        f = c - b[:, None, 3:]
        e = np.where(f > e, f, e)
        e = np.where(e > 0, e, R(0.0))
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        gap = np.sqrt(dd) - np.sqrt(np.where(rr > 0, rr, R(1.0)))[None, :]
    return np.where((rr > 0)[None, :], gap, R(np.inf)).astype(R, copy=False)


ABSENT_PLANE = (0.0, 0.0, 0.0, -np.inf)


def _as_regions(planes, what="planes"):
    """`planes` as (n, 24) in its own float dtype: (n, 6, 4) or (n, 24) in."""
    p = np.asarray(planes)
    if p.dtype not in (np.float32, np.float64) or not ((p.ndim == 3 and p.shape[1:] == (6, 4)) or (p.ndim == 2 and p.shape[1] == 24)):
        raise ValueError("%s must be (n, 6, 4) or (n, 24), float32 or float64" % what)
    return p.reshape(p.shape[0], 24)


def region_gaps(planes, spheres):
    """The gap between every convex region of `planes` (n x 6 x 4 or n x 24: six planes {n.x, n.y, n.z, d}; outside is n.c + d > 0) and every
    sphere of `spheres` (m x 4: cx, cy, cz, r) -> REAL[n, m], the metric of rt_overlap_regions restated in numpy bit for bit
    (include/rtrace_hip.h states it), in the arrays' dtype (float32 or float64, the same for both), every operation rounded once:
    rr = r * r;  s_k = ((n_k.x*c.x + n_k.y*c.y) + n_k.z*c.z) + d_k;  m = -inf, then m = s_k where s_k > m, k = 0 .. 5;  gap = m - sqrt(rr)
    where rr > 0, else +inf.  With unit normals: the largest signed plane distance of the centre, minus the radius -- never above the
    true distance from the region to the sphere's surface.  An absent plane is (0, 0, 0, -inf).  A record without a positive rr -- radius
    0: a dead slot -- is at +inf from every region.  DeviceScene.region_overlaps lists, per region without a NaN, the spheres with
    !(gap >= margin); the row of a region with a NaN is here whatever the arithmetic gives."""
    try:
        p = _as_regions(planes)
    except ValueError:
        p = None
    s = np.asarray(spheres)
    if p is None or s.dtype != p.dtype or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("planes must be (n, 6, 4) or (n, 24) and spheres (m, 4), both float32 or both float64")
    R = p.dtype.type
    rr = s[:, 3] * s[:, 3]
    m = np.full((p.shape[0], s.shape[0]), -np.inf, dtype=R)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(6):
            nx, ny, nz, d = (p[:, 4 * k + c, None] for c in range(4))
            sk = ((nx * s[None, :, 0] + ny * s[None, :, 1]) + nz * s[None, :, 2]) + d
            m = np.where(sk > m, sk, m)
        gap = m - np.sqrt(np.where(rr > 0, rr, R(1.0)))[None, :]
    return np.where((rr > 0)[None, :], gap, R(np.inf)).astype(R, copy=False)


def _unit_planes(normals, points, dtype):
    """REAL[..., 4] = {n / |n|, -(n / |n|) . p}: normalised in float64, rounded to `dtype` once."""
    nrm = np.asarray(normals, dtype=np.float64)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
    d = -(nrm * np.asarray(points, dtype=np.float64)).sum(axis=-1, keepdims=True)
    return np.concatenate([nrm, d], axis=-1).astype(dtype)


def box_planes(lo, hi, rotation=None, dtype=None):
    """The six unit planes of the box [lo, hi] for DeviceScene.region_overlaps -> REAL[n, 6, 4] (lo, hi: (n, 3) or (3,), float32 or float64;
    dtype: the result's, default lo's).  rotation=None: the axis-aligned box; rotation (3 x 3, or n x 3 x 3, orthonormal): the box
    {c + rotation @ x : lo <= c + x <= hi componentwise} -- the box turned about its own centre c = (lo + hi) / 2, the rotation's columns
    its axes.  Planes 2k and 2k + 1 are the low and the high side of axis k: {-a_k, a_k . c - h_k} and {a_k, -a_k . c - h_k} with h the
    half-extents.  An infinite side becomes the absent plane (0, 0, 0, -inf) (with a rotation, only where the centre of that axis is
    still finite: a box infinite on both sides of a rotated axis has no centre to turn about and is refused).  Formed in float64, rounded
    to REAL once.  For an axis-aligned box region_gaps <= box_gaps: the largest excess is never above the root of the squares' sum."""
    lo_a = np.asarray(lo)
    R = np.dtype(dtype if dtype is not None else lo_a.dtype).type
    if R not in (np.float32, np.float64):
        raise ValueError("box_planes: lo and hi must be float32 or float64 (or pass dtype)")
    lo64, hi64 = np.atleast_2d(np.asarray(lo, np.float64)), np.atleast_2d(np.asarray(hi, np.float64))
    if lo64.shape != hi64.shape or lo64.ndim != 2 or lo64.shape[1] != 3 or np.isnan(lo64).any() or np.isnan(hi64).any() or (lo64 > hi64).any():
        raise ValueError("box_planes: lo and hi must be (n, 3) or (3,) without NaN and with lo <= hi")
    n = lo64.shape[0]
    out = np.empty((n, 6, 4), dtype=R)
    if rotation is None:
        axes = np.broadcast_to(np.eye(3), (n, 3, 3))
        for k in range(3):
            out[:, 2 * k, :3] = -axes[:, :, k]
            out[:, 2 * k, 3] = lo64[:, k]                                       # -c_k + lo_k <= 0
            out[:, 2 * k + 1, :3] = axes[:, :, k]
            out[:, 2 * k + 1, 3] = -hi64[:, k]
    else:
        rot = np.broadcast_to(np.asarray(rotation, dtype=np.float64), (n, 3, 3))
        if not np.allclose(np.einsum("nij,nik->njk", rot, rot), np.eye(3), atol=1e-9):
            raise ValueError("box_planes: rotation must be orthonormal")
        fin = np.isfinite(lo64) & np.isfinite(hi64)
        if (np.isinf(lo64) & np.isinf(hi64)).any():
            raise ValueError("box_planes: a rotated box must have a finite side on every axis")
        with np.errstate(invalid="ignore"):
            c = np.where(fin, 0.5 * (lo64 + hi64), np.where(np.isfinite(lo64), lo64, hi64))     # (a half-infinite axis turns about its finite side)
        below, above = np.where(np.isfinite(lo64), lo64 - c, 0.0), np.where(np.isfinite(hi64), hi64 - c, 0.0)     # (an infinite side: absent below)
        for k in range(3):
            a = rot[:, :, k]
            out[:, 2 * k] = _unit_planes(-a, c + a * below[:, k, None], R)
            out[:, 2 * k + 1] = _unit_planes(a, c + a * above[:, k, None], R)
    for k in range(3):
        out[np.isinf(lo64[:, k]), 2 * k] = ABSENT_PLANE
        out[np.isinf(hi64[:, k]), 2 * k + 1] = ABSENT_PLANE
    return out + R(0.0)                                                          # (no component is a negative zero)


def camera_planes(camera, width, height, rect=None, near=None, far=None):
    """The planes that enclose what a look_at camera sees through a pixel rectangle, for DeviceScene.region_overlaps -> REAL[1, 6, 4] in the
    camera's dtype.  camera: REAL[12] = eye, right, up, forward (look_at); width, height: the frame's; rect = (l, t, r, b): the pixels
    l <= x < r, b <= y < t as render_camera's regions name them (None: the whole frame).
    Planes 0 .. 3 are the four sides through the eye.  render_camera's sample (x, y, ssx, ssy) looks along (right*u + up*v) + forward*width
    with u = xres - width/2, v = (height - yres) - height/2, x <= xres < x + 1 and y <= yres < y + 1 (include/rtrace_hip.h): the
    rectangle's samples have u in [l - width/2, r - width/2] and v in [(height - t) - height/2, (height - b) - height/2].  Both ranges
    are rounded outward to whole numbers and then widened by one pixel more on every side, so that the planes' own rounding to REAL never
    puts a sample ray outside: every point eye + t*dir, t >= 0, of every sample ray has s_k < 0 on all four sides at any t > 0.  In
    the camera's (possibly skewed) axes a direction right*a + up*b + forward*c lies inside u <= u1 exactly when width*a - u1*c <= 0,
    which is a plane through the eye whose normal is read off the dual basis; all four normals are normalised in float64 and rounded to
    REAL once.  Plane 4 is the near plane (points closer than `near` along forward / |forward| are outside), plane 5 the far plane;
    None leaves them absent, (0, 0, 0, -inf)."""
    cam = np.asarray(camera)
    if cam.dtype not in (np.float32, np.float64) or cam.shape != (12,):
        raise ValueError("camera_planes: camera must be float32[12] or float64[12] (look_at)")
    R = cam.dtype.type
    w, h = int(width), int(height)
    l, t, r, b = (0, h, w, 0) if rect is None else (int(v) for v in rect)
    if not (w > 0 and h > 0 and 0 <= l < r <= w and 0 <= b < t <= h):
        raise ValueError("camera_planes: rect (l, t, r, b) must be a non-empty rectangle inside the %dx%d frame" % (w, h))
    c64 = cam.astype(np.float64)
    eye, axes = c64[:3], c64[3:].reshape(3, 3)                                  # rows: right, up, forward
    dual = np.linalg.inv(axes.T)                                                # rows: a(d) = dual[0] . d, b(d) = dual[1] . d, c(d) = dual[2] . d
    u0, u1 = np.floor(l - w / 2.0) - 1.0, np.ceil(r - w / 2.0) + 1.0
    v0, v1 = np.floor((h - t) - h / 2.0) - 1.0, np.ceil((h - b) - h / 2.0) + 1.0
    normals = [u0 * dual[2] - w * dual[0], w * dual[0] - u1 * dual[2], v0 * dual[2] - w * dual[1], w * dual[1] - v1 * dual[2]]
    out = np.empty((1, 6, 4), dtype=R)
    out[0, :4] = _unit_planes(np.array(normals), eye[None, :], R)
    f = axes[2] / np.sqrt(axes[2] @ axes[2])
    out[0, 4] = ABSENT_PLANE if near is None else _unit_planes(-f, eye + f * float(near), R)
    out[0, 5] = ABSENT_PLANE if far is None else _unit_planes(f, eye + f * float(far), R)
    return out + R(0.0)


REGION_LANES, REGION_SECTION_NODES, REGION_MAX_COUNTS = 1 << 18, 8, 1 << 26


def region_sections(n, n_nodes, sections=0):
    """The J of an rt_overlap_regions call over n regions on a stream of n_nodes nodes (a scene without bounds: its items) -- sections=0:
    the library's rule, a pure function of (n, n_nodes): max(1, min(2^18 // n, n_nodes // 8)) -- as many sections as bring the call to
    2^18 lanes, none shorter than 8 nodes (DESIGN.md 4.23 has the sweep that chose the constants); any other value: clamped to
    1 .. n_nodes, as the library clamps it."""
    n, n_nodes, sections = int(n), max(int(n_nodes), 1), int(sections)
    if n < 1 or sections < 0:
        raise ValueError("region_sections: n must be >= 1 and sections >= 0")
    return max(1, min(REGION_LANES // n, n_nodes // REGION_SECTION_NODES)) if sections == 0 else min(sections, n_nodes)


def impact_scale(spheres, disp, queries=None, qdisp=None):
    """S of rt_scene_impacts (include/rtrace_hip.h) for the records `spheres` (m x 4: cx, cy, cz, r) and their motion-table rows `disp`
    (m x 3, or None: 0) -> a power of two in the arrays' dtype.  M is the largest of |cx|, |cy|, |cz|, r, |dx|, |dy|, |dz| over the records
    with a positive rr -- the library takes it over the nodes of the scene's stream, bounds included (a bound's row is 0) -- and
    S = 2^-e, M = f 2^e with 0.5 <= f < 1, e held to [MIN_EXP + 1, MAX_EXP - 2] so that S is a normal number; S = 1 when M is 0.
    Every scaled magnitude is then below 1.  `queries` (n x 4: px, py, pz, q) with `qdisp` (n x 3) gives S of rt_swept_overlaps: M also
    covers |px|, |py|, |pz|, q, |dqx|, |dqy|, |dqz| over the queries with q >= 0."""
    s = np.asarray(spheres)
    R = s.dtype.type
    d = np.zeros((s.shape[0], 3), R) if disp is None else np.asarray(disp)
    with np.errstate(over="ignore", under="ignore"):
        rr = s[:, 3] * s[:, 3]
    solid = rr > 0
    M = 0.0
    if solid.any():
        M = max(float(np.abs(s[solid, :3]).max()), float(np.abs(s[solid, 3]).max()), float(np.abs(d[solid]).max()))
    if queries is not None:
        qs, qd = np.asarray(queries), np.asarray(qdisp)
        with np.errstate(invalid="ignore"):
            carried = qs[:, 3] >= 0
        if carried.any():
            M = max(M, float(np.abs(qs[carried, :3]).max()), float(qs[carried, 3].max()), float(np.abs(qd[carried]).max()))
    M = R(M)
    if not M > 0:
        return R(1.0)
    fi = np.finfo(R)
    e = min(max(int(np.frexp(M)[1]), fi.minexp + 1), fi.maxexp - 2)
    return R(np.ldexp(1.0, -e))


def pair_impacts(spheres, disp, i, j, inflate=None, scale=None):
    """The time of impact of the pairs (i[k], j[k]) of `spheres` (m x 4: cx, cy, cz, r) that move by `disp` (m x 3) during one step -- sphere
    k is at c_k + t d_k for t in [0, 1] -> REAL[len(i)], the metric of rt_scene_impacts restated in numpy bit for bit (include/rtrace_hip.h
    states it), in the arrays' dtype (float32 or float64), every operation rounded once.  Every input is first multiplied by S, a power
    of two that brings the whole scene below 1 (impact_scale; `scale`: that of another set of records, None: impact_scale(spheres, disp)):
    rr = r * r;  c' = c S;  r' = r S;  d' = d S;  E' = E S;  v = c_j' - c_i';  w = d_i' - d_j';  R = (r_j' + E_j') + r_i';
    a = dot(w, w), b = dot(v, w), c = dot(v, v) - R * R, disc = b*b - a*c;  t = +inf where not (rr_i > 0 and rr_j > 0), else 0 where
    not c > 0 (in contact at the start), else +inf where not b > 0 or disc < 0 (not approaching, or passing by), else
    c / (b + sqrt(disc)).  t has no dimension and the products with S are exact, so S changes no bit of t as long as nothing leaves the
    normal range -- which is what S is for: a, b and c are of the second degree in a length, disc of the fourth.  The library always
    takes the lower slot as i.  `inflate` (REAL[m] or None: 0) is E, what the walk adds to the radius of a BOUND record: 0 for every item.
    A record without a positive rr -- radius 0: a dead slot -- is at +inf, in either place, and does not contribute to S.
    DeviceScene.impacts lists the pairs i < j with t <= 1."""
    s, d = np.asarray(spheres), np.asarray(disp)
    if s.dtype not in (np.float32, np.float64) or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("spheres must be an (m, 4) array of float32 or float64")
    if d.dtype != s.dtype or d.shape != (s.shape[0], 3):
        raise ValueError("disp must be an (m, 3) array of the spheres' dtype")
    R = s.dtype.type
    E = np.zeros(s.shape[0], R) if inflate is None else np.asarray(inflate)
    if E.dtype != s.dtype or E.shape != (s.shape[0],):
        raise ValueError("inflate must be None or an (m,) array of the spheres' dtype")
    i, j = np.asarray(i), np.asarray(j)
    if i.dtype.kind not in "iu" or j.dtype.kind not in "iu" or i.ndim != 1 or i.shape != j.shape:
        raise ValueError("i and j must be integer arrays of one shape, (k,)")
    if i.size and (min(int(i.min()), int(j.min())) < 0 or max(int(i.max()), int(j.max())) >= s.shape[0]):
        raise ValueError("i and j must be rows of spheres")
    S = impact_scale(s, d) if scale is None else R(scale)
    if not (S > 0 and np.isfinite(S) and np.frexp(S)[0] == 0.5):
        raise ValueError("scale must be a positive power of two")
    with np.errstate(over="ignore", under="ignore"):
        rr = s[:, 3] * s[:, 3]
    rri, rrj = rr[i], rr[j]
    solid = (rri > 0) & (rrj > 0)
    one = R(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        cs, d, E = s[:, :3] * S, d * S, E * S
        v = cs[j] - cs[i]
        w = d[i] - d[j]
        r = np.abs(s[:, 3]) * S
        rad = (r[j] + E[j]) + r[i]
        RR = rad * rad
        a = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        b = (v[:, 0] * w[:, 0] + v[:, 1] * w[:, 1]) + v[:, 2] * w[:, 2]
        c = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) - RR
        disc = b * b - a * c
        root = (b > 0) & ~(disc < 0)
        t = np.where(root, c / (b + np.sqrt(np.where(root, disc, one))), R(np.inf))
        t = np.where(c > 0, t, R(0.0))
    return np.where(solid, t, R(np.inf)).astype(R, copy=False)


def pair_islands(pairs, n_items, live=None):
    """The islands of the graph on `n_items` slots with the edges `pairs` (m x 2 integers, each a pair of slots; any order, repeats
    allowed) -> (label int32[n_items], index int32[n_items], size uint32[n_items], n_islands), the definition of rt_scene_islands and
    rt_scene_impact_islands restated in numpy (include/rtrace_hip.h states it): label[i] is the smallest slot of i's connected component,
    index[i] the number of islands whose label is below label[i] (dense, 0 .. n_islands - 1, ascending in the label), size[i] the slots
    of i's island, n_islands the number of i with label[i] == i.  live (bool or uint8 [n_items], or None: every slot): a slot that is
    not live belongs to no island -- label -1, index -1, size 0 -- and must be in no pair.  A live slot in no pair is an island of one.
    With the pairs of DeviceScene.contacts(margin), or of impacts(disp), and the scene's live slots this is what islands(margin), or
    impact_islands(disp), returns."""
    n = int(n_items)
    if n < 0:
        raise ValueError("n_items must not be negative")
    p = np.asarray(pairs)
    if p.size == 0:
        p = np.zeros((0, 2), np.int64)
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("pairs must be an (m, 2) integer array")
    p = p.astype(np.int64)
    if p.size and (int(p.min()) < 0 or int(p.max()) >= n):
        raise ValueError("pairs must name slots 0 .. n_items - 1")
    if live is None:
        alive = np.ones(n, bool)
    else:
        alive = np.asarray(live)
        if alive.dtype not in (np.uint8, np.bool_) or alive.shape != (n,):
            raise ValueError("live must be None or an (n_items,) array of uint8 or bool")
        alive = alive != 0
    if not alive[p].all():
        raise ValueError("a pair names a slot that is not live")
    i, j = p[:, 0], p[:, 1]
    parent = np.arange(n, dtype=np.int64)
    while True:                                  # every tree is flat here: parent[x] is x's root, and a root is its tree's smallest slot
        ri, rj = parent[i], parent[j]
        lo, hi = np.minimum(ri, rj), np.maximum(ri, rj)
        apart = lo != hi
        if not apart.any():
            break
        np.minimum.at(parent, hi[apart], lo[apart])                          # the higher root goes below the lowest root it has an edge to
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    label = np.where(alive, parent, -1).astype(np.int32)
    root = label == np.arange(n)
    rank = np.cumsum(root) - 1
    index = np.where(alive, rank[parent], -1).astype(np.int32)
    members = np.bincount(parent[alive], minlength=n) if n else np.zeros(0, np.int64)
    size = np.where(alive, members[parent], 0).astype(np.uint32)
    return label, index, size, int(root.sum())


def _swept_terms(queries, qdisp, spheres, disp, inflate, scale):
    """(t, v, w) of swept_times: REAL[n, m], REAL[n, m, 3], REAL[n, m, 3]."""
    qs, qd, s = np.asarray(queries), np.asarray(qdisp), np.asarray(spheres)
    if qs.dtype not in (np.float32, np.float64) or qs.ndim != 2 or qs.shape[1] != 4:
        raise ValueError("queries must be an (n, 4) array of float32 or float64")
    if qd.dtype != qs.dtype or qd.shape != (qs.shape[0], 3):
        raise ValueError("qdisp must be an (n, 3) array of the queries' dtype")
    if s.dtype != qs.dtype or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("spheres must be an (m, 4) array of the queries' dtype")
    R = qs.dtype.type
    d = np.zeros((s.shape[0], 3), R) if disp is None else np.asarray(disp)
    if d.dtype != s.dtype or d.shape != (s.shape[0], 3):
        raise ValueError("disp must be None or an (m, 3) array of the queries' dtype")
    E = np.zeros(s.shape[0], R) if inflate is None else np.asarray(inflate)
    if E.dtype != s.dtype or E.shape != (s.shape[0],):
        raise ValueError("inflate must be None or an (m,) array of the queries' dtype")
    S = impact_scale(s, d, qs, qd) if scale is None else R(scale)
    if not (S > 0 and np.isfinite(S) and np.frexp(S)[0] == 0.5):
        raise ValueError("scale must be a positive power of two")
    one = R(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        rr = s[:, 3] * s[:, 3]
        cs, ds, Es, r = s[:, :3] * S, d * S, E * S, np.abs(s[:, 3]) * S
        ps, dqs, q = qs[:, :3] * S, qd * S, qs[:, 3] * S
        v = cs[None, :, :] - ps[:, None, :]
        w = dqs[:, None, :] - ds[None, :, :]
        rad = (r + Es)[None, :] + q[:, None]
        RR = rad * rad
        a = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
        b = (v[..., 0] * w[..., 0] + v[..., 1] * w[..., 1]) + v[..., 2] * w[..., 2]
        c = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) - RR
        disc = b * b - a * c
        root = (b > 0) & ~(disc < 0)
        t = np.where(root, c / (b + np.sqrt(np.where(root, disc, one))), R(np.inf))
        t = np.where(c > 0, t, R(0.0))
    return np.where((rr > 0)[None, :], t, R(np.inf)).astype(R, copy=False), v, w


def swept_times(queries, qdisp, spheres, disp=None, inflate=None, scale=None):
    """The time at which every moving query sphere of `queries` (n x 4: px, py, pz, q; query g is at p + t qdisp[g] for t in [0, 1]) first
    touches every sphere of `spheres` (m x 4: cx, cy, cz, r) that moves by `disp` (m x 3, or None: it stands still) -> REAL[n, m], the metric
    of rt_swept_overlaps restated in numpy bit for bit (include/rtrace_hip.h states it), in the arrays' dtype (float32 or float64, the same
    for all), every operation rounded once.  Every input is first multiplied by S, a power of two (`scale`, or None: impact_scale over
    everything given here -- spheres, disp, queries and qdisp): rr = r * r;  p' = p S, q' = q S, dq' = dq S, c' = c S, r' = |r| S, d' = d S,
    E' = E S;  v = c' - p';  w = dq' - d';  R = (r' + E') + q';  a = dot(w, w), b = dot(v, w), cc = dot(v, v) - R * R, disc = b*b - a*cc;
    t = +inf where not rr > 0, else 0 where not cc > 0 (in contact at the start), else +inf where not b > 0 or disc < 0 (not
    approaching, or passing by), else cc / (b + sqrt(disc)).  pair_impacts with the query in the place of sphere i -- for q > 0 the
    same bits as pair_impacts over the concatenated records -- but q = 0 is a query here: a moving point.  `inflate` (REAL[m] or None: 0)
    is E, what the walk adds to the radius of a BOUND record.  A record without a positive rr -- radius 0: a dead slot -- is at +inf and
    does not contribute to S.  DeviceScene.swept_overlaps lists, per query with q >= 0, the spheres with t <= 1; a query whose q is not
    >= 0 carries no query there and does not contribute to S; its row here is whatever the arithmetic gives."""
    return _swept_terms(queries, qdisp, spheres, disp, inflate, scale)[0]


def swept_normals(queries, qdisp, spheres, disp=None, inflate=None, scale=None):
    """The contact normal rt_swept_overlaps reports for every (query, sphere) of swept_times -> REAL[n, m, 3], bit for bit: u = w * t - v
    (each product and difference rounded once) -- the query's centre minus the sphere's centre at time t, in the scaled frame --
    then u * (1 / sqrt(dot(u, u))): from the touched sphere to the query.  NaN where t is not finite, and where the centres coincide
    (u = 0)."""
    t, v, w = _swept_terms(queries, qdisp, spheres, disp, inflate, scale)
    R = t.dtype.type
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        u = w * t[..., None] - v
        ln = np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
        rc = R(1.0) / ln
        return (u * rc[..., None]).astype(R, copy=False)


def sweep_distances(rays, radius, spheres):
    """The cast distance of every cast of `rays` (n x 6: pos.xyz, dir.xyz, dir a unit vector) with `radius` (REAL[n], one value, or None: 0)
    against every sphere of `spheres` (m x 4: cx, cy, cz, r) -> REAL[n, m], the metric of rt_sweep_spheres restated in numpy bit for bit
    (include/rtrace_hip.h states it), in the arrays' dtype (float32 or float64, the same for all), every operation rounded once:
    rr = r * r;  rad = sqrt(rr);  RR = (rr + (q + q) * rad) + q * q;  v = c - pos;  b = dot(v, dir);  disc = (b*b - dot(v, v)) + RR;
    t = +inf where !(rr > 0), disc < 0 or b + sqrt(disc) < 0, else b - sqrt(disc) where that is > 0, else 0 (the moving sphere touches
    or overlaps the sphere at its start).  A record without a positive rr -- radius 0: a dead slot, a dead group's bound -- is at +inf
    from every cast, as in sphere_gaps.  DeviceScene.sweep reports, per cast, the smallest of a row below tmax as its walk finds it."""
    ry, s = np.asarray(rays), np.asarray(spheres)
    if ry.dtype not in (np.float32, np.float64) or s.dtype != ry.dtype or ry.ndim != 2 or ry.shape[1] != 6 or s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("rays must be (n, 6) and spheres (m, 4), both float32 or both float64")
    R = ry.dtype.type
    n = ry.shape[0]
    q = np.zeros(n, R) if radius is None else np.asarray(radius)
    if q.ndim == 0 and q.dtype.kind in "fiu":
        q = q.astype(R)
    if q.dtype != R or q.size not in (1, n):
        raise ValueError("radius must be None, one value or an (n,) array of %s" % np.dtype(R).name)
    q = np.broadcast_to(q.reshape(-1), (n,))
    rr = s[:, 3] * s[:, 3]
    solid = rr > 0
    with np.errstate(invalid="ignore", over="ignore"):
        rad = np.sqrt(np.where(solid, rr, R(1.0)))
        RR = (rr[None, :] + (q + q)[:, None] * rad[None, :]) + (q * q)[:, None]
        v = s[None, :, :3] - ry[:, None, :3]
        d = ry[:, None, 3:]
        b = (v[..., 0] * d[..., 0] + v[..., 1] * d[..., 1]) + v[..., 2] * d[..., 2]
        vv = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        disc = (b * b - vv) + RR
        root = np.sqrt(np.where(disc < 0, R(0.0), disc))
        hit = solid[None, :] & ~(disc < 0) & ~(b + root < 0)
        t1 = b - root
        t = np.where(hit, np.where(t1 > 0, t1, R(0.0)), R(np.inf))
    return t.astype(R, copy=False)


def balanced_ranges(n, leaf_size=4):
    """rt_balanced_ranges: a topology from the item count alone -> int32[g, 2], the groups (first item, item count) of the recursive halving
    of (0, n) down to `leaf_size`, in DFS pre-order (a group's first half holds (count + 1) // 2 items; leaves are groups too).  Valid as
    the `ranges` of a Scene as it stands; over spheres in the sphere order it is a median-split tree along the Morton curve, which is what
    DeviceScene.rebuild keeps a dynamic scene in.  balanced_ranges_reference restates it in numpy."""
    n, leaf_size = int(n), int(leaf_size)
    if not 0 <= n <= 0xFFFFFFFF or not 0 <= leaf_size <= 0xFFFFFFFF:
        raise ValueError("n and leaf_size must fit 32 bits")
    ranges = np.zeros((2 * max(n, 1), 2), dtype=np.int32)
    ng = C.c_uint32(0)
    capi.check(capi.lib.rt_balanced_ranges(n, leaf_size, ranges.ctypes.data, C.byref(ng)), "rt_balanced_ranges")
    return ranges[:int(ng.value)].copy()


def balanced_ranges_reference(n, leaf_size=4):
    """The rule of rt_balanced_ranges in plain Python (test infrastructure).  Same return value as balanced_ranges."""
    if n < 1 or leaf_size < 1:
        raise ValueError("balanced_ranges needs at least one item and a leaf size of at least 1")
    out = []

    def emit(first, count):
        out.append((first, count))
        if count > leaf_size:
            left = (count + 1) // 2
            emit(first, left)
            emit(first + left, count - left)

    emit(0, int(n))
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def refit_bounds(items, ranges, precision=capi.RT_F32, bounds=None, live=None):
    """The bounds rt_scene_update refits for `items` (n x 4: cx, cy, cz, r) over `ranges` (g x 2: first item, item count) -> REAL[g, 4],
    the rule of include/rtrace_hip.h restated in numpy bit for bit: every operation in REAL, rounded once.  Per group: lo / hi = min / max
    of c -+ r, centre = (lo + hi) * 0.5, reach = dist(c, centre) + r with dist = sqrt((dx*dx + dy*dy) + dz*dz), or (|dx| + |dy|) + |dz|
    where that sum of squares is below MIN_NORMAL / EPSILON^2, radius = max(reach) * (1 + 8 * EPSILON).  A group without items keeps its
    row of `bounds` (zeros when there is none).  live (n values, nonzero = live; None: all): the rule over each group's LIVE items only,
    as rt_scene_update_live refits -- the values in dead slots take no part, NaN included, and a group without a live item gets
    {0, 0, 0, 0}."""
    R = _real(precision)
    it = np.ascontiguousarray(items, dtype=R).reshape(-1, 4)
    alive = None
    if live is not None:
        alive = np.asarray(live).reshape(-1) != 0
        if alive.shape[0] != it.shape[0]:
            raise ValueError("live must have one value per item")
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((rg.shape[0], 4), dtype=R) if bounds is None else np.array(bounds, dtype=R).reshape(-1, 4)
    if out.shape[0] != rg.shape[0]:
        raise ValueError("bounds must have one row per range")
    tiny = np.ldexp(R(1.0), -80 if R == np.float32 else -918)          # MIN_NORMAL / EPSILON^2
    grow = R(1.0) + R(8.0) * np.finfo(R).eps
    half = R(0.5)
    c, r = it[:, :3], it[:, 3]
    lo_all, hi_all = c - r[:, None], c + r[:, None]
    for g in range(rg.shape[0]):
        first, count = int(rg[g, 0]), int(rg[g, 1])
        if first < 0 or count < 0 or first + count > it.shape[0]:
            raise ValueError("range %d lies outside the items" % g)
        if count == 0:
            continue
        sl = slice(first, first + count)
        if alive is not None:
            sl = first + np.flatnonzero(alive[sl])
            if sl.size == 0:
                out[g] = 0
                continue
        centre = (lo_all[sl].min(axis=0) + hi_all[sl].max(axis=0)) * half
        d = c[sl] - centre
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        a = np.abs(d)
        dist = np.where(s >= tiny, np.sqrt(s), (a[:, 0] + a[:, 1]) + a[:, 2])
        out[g, :3] = centre
        out[g, 3] = (dist + r[sl]).max() * grow
    return out


def pyramid(level, origin, radius, precision=capi.RT_F32):
    """SphericalGroup::pyramid (group.rs:58-65) -> (items REAL[n,4], bounds REAL[g,4], ranges int32[g,2]).

    items are in traversal order (own sphere first, then the four sub-pyramids, dz outer / dx inner,
    group.rs:39-53); bounds/ranges are in DFS pre-order with ranges[i] = (first item, item count) of the subtree."""
    if level <= 1:
        raise ValueError("Levels equal or smaller than one cause empty groups")      # group.rs:59-60
    R = _real(precision)
    three, half, s12 = R(3.0), R(0.5), np.sqrt(R(12.0))
    items, bounds, ranges = [], [], []

    def rec(lv, px, py, pz, r):
        if lv == 1:
            items.append((px, py, pz, r))
            return
        bi = len(bounds)
        bounds.append((px, py, pz, three * r))          # group.rs:40-41
        ranges.append(None)
        first = len(items)
        items.append((px, py, pz, r))                   # group.rs:39
        rn = three * r / s12                            # group.rs:43
        for dz in (-1, 1):
            for dx in (-1, 1):
                rec(lv - 1, px + R(dx) * rn, py + rn, pz + R(dz) * rn, r * half)
        ranges[bi] = (first, len(items) - first)

    rec(level, R(origin[0]), R(origin[1]), R(origin[2]), R(radius))
    return (np.array(items, dtype=R).reshape(-1, 4), np.array(bounds, dtype=R).reshape(-1, 4),
            np.array(ranges, dtype=np.int32).reshape(-1, 2))


def normalized(v, precision=capi.RT_F32):
    """Vector::normalized (vec.rs:92-95): v * (1/len), len = sqrt((x*x + y*y) + z*z)."""
    R = _real(precision)
    x, y, z = R(v[0]), R(v[1]), R(v[2])
    ln = np.sqrt((x * x + y * y) + z * z)
    rc = R(1.0) / ln
    return np.array([x * rc, y * rc, z * rc], dtype=R)


def look_at(eye, target, up=(0.0, 1.0, 0.0), hfov_deg=None, precision=capi.RT_F32):
    """A camera for DeviceScene.render_camera -> REAL[12] = eye, right, up, forward, formed in double and rounded to REAL once:
    forward = normalize(target - eye), right = normalize(cross(up, forward)), up' = cross(forward, right).  hfov_deg: the horizontal
    field of view, by scaling forward to 0.5 / tan(hfov / 2); None keeps |forward| = 1, the reference's view (2 * atan(0.5), about 53.13
    degrees).  look_at((0, 0, -4), (0, 0, 0)) is the identity camera of the default eye.  ValueError when eye == target or when up is
    parallel to the view."""
    e, t, u = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    f = t - e
    fl = float(np.sqrt(f @ f))
    if not fl > 0.0 or not np.isfinite(fl):
        raise ValueError("look_at: eye and target must be distinct finite points")
    f = f / fl
    r = np.cross(u, f)
    rl = float(np.sqrt(r @ r))
    ul = float(np.sqrt(u @ u))
    if not rl > 1e-9 * ul:
        raise ValueError("look_at: up is parallel to the view direction (or zero)")
    r = r / rl
    u2 = np.cross(f, r)
    if hfov_deg is not None:
        if not 0.0 < hfov_deg < 180.0:
            raise ValueError("look_at: hfov_deg must lie in (0, 180)")
        f = f * (0.5 / np.tan(np.radians(hfov_deg) / 2.0))
    # (+ 0.0: no axis component is a negative zero)
    return np.concatenate([e, r + 0.0, u2 + 0.0, f + 0.0]).astype(_real(precision))


def expand_undersampled(image, regions, step):
    """The step-s frame of `regions`, from the full image: every pixel (x, y) of every region holds image[y - y % step, x - x % step] (the
    lattice is anchored at the image origin, so an anchor may lie outside its region).  image: uint8[height, width, 4] row-major, what
    render_camera returns for the single region (0, height, width, 0); regions: (l, t, r, b) tuples.  -> uint8[total_px * 4] tile-major,
    the bytes render_camera_undersampled(step) writes.  Host only (numpy)."""
    img = np.asarray(image)
    step = int(step)
    if img.ndim != 3 or img.shape[2] != 4 or img.dtype != np.uint8:
        raise ValueError("image must be uint8[height, width, 4]")
    if step < 1:
        raise ValueError("step must be >= 1")
    h, w = img.shape[:2]
    parts = []
    for l, t, r, b in regions:
        if not (0 <= l < r <= w and 0 <= b < t <= h):
            raise ValueError("region %r is empty or outside the %dx%d image" % ((l, t, r, b), w, h))
        ys, xs = np.arange(b, t), np.arange(l, r)
        parts.append(img[(ys - ys % step)[:, None], (xs - xs % step)[None, :]].reshape(-1))
    return np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)


def undersample_cells(regions, step, prev_step=0):
    """(traced, reused) cells of one render_camera_undersampled pass: over the regions, the step-s cells that meet a region and are traced
    (all of them when prev_step == 0; with prev_step == 2 * step those whose anchor is off the 2s lattice) and those that are kept."""
    step = int(step)
    if prev_step not in (0, 2 * step):
        raise ValueError("prev_step must be 0 or 2 * step")
    traced = reused = 0
    for l, t, r, b in regions:
        nx, ny = (r - 1) // step - l // step + 1, (t - 1) // step - b // step + 1
        kept = 0
        if prev_step:      # cells (cx, cy) with cx and cy even: the even numbers of [a, b] are b // 2 - (a + 1) // 2 + 1
            kept = ((r - 1) // step // 2 - (l // step + 1) // 2 + 1) * ((t - 1) // step // 2 - (b // step + 1) // 2 + 1)
        traced += nx * ny - kept
        reused += kept
    return traced, reused


def progressive_steps(first_step):
    """[first_step, first_step / 2, ..., 1] for a power of two first_step <= RT_UNDERSAMPLE_MAX_STEP; ValueError otherwise."""
    if isinstance(first_step, bool) or not isinstance(first_step, (int, np.integer)) or first_step < 1 \
            or first_step > capi.RT_UNDERSAMPLE_MAX_STEP or first_step & (first_step - 1):
        raise ValueError("first_step must be a power of two in 1 .. %d, not %r" % (capi.RT_UNDERSAMPLE_MAX_STEP, first_step))
    steps = []
    s = int(first_step)
    while s >= 1:
        steps.append(s)
        s //= 2
    return steps


def build_hierarchy(spheres, leaf_size=4, precision=capi.RT_F32, eye=None):
    """Bounding-sphere hierarchy for an arbitrary sphere list (scenes other than the pyramid, e.g. BASELINE
    config 5 with exactly 100,000 spheres).  Not in the reference -- its only scene builder is `pyramid` -- but the result
    is an ordinary `TypedGroup` tree in the flat description the C ABI takes: median splits along the longest axis until
    at most `leaf_size` spheres remain; every group's bound is a near-minimal enclosing sphere of its whole subtree (inflated
    by 1e-4 so that it also encloses after rounding to REAL); with `eye`, a group's nearer half comes first.

    ONE implementation for both hosts: csrc/host/hierarchy.hpp, here through the library's rt_build_hierarchy (no device is
    touched).  build_hierarchy_reference below restates the same arithmetic in numpy; the tests hold one against the other.

    Returns (items REAL[n,4] in the tree's DFS order, bounds REAL[g,4], ranges int32[g,2], order int64[n]) where
    items == spheres[order]."""
    R = _real(precision)
    sp = np.ascontiguousarray(np.asarray(spheres, dtype=np.float64).reshape(-1, 4))
    n = sp.shape[0]
    if n == 0:
        raise ValueError("build_hierarchy needs at least one sphere")
    items = np.zeros((n, 4), dtype=R)
    bounds = np.zeros((2 * n, 4), dtype=R)
    ranges = np.zeros((2 * n, 2), dtype=np.int32)
    order = np.zeros(n, dtype=np.uint64)
    ng = C.c_uint32(0)
    e = None if eye is None else np.ascontiguousarray(np.asarray(eye, dtype=np.float64).reshape(3))
    capi.check(capi.lib.rt_build_hierarchy(sp.ctypes.data, n, int(leaf_size), None if e is None else e.ctypes.data, precision, items.ctypes.data,
                                           bounds.ctypes.data, ranges.ctypes.data, order.ctypes.data, C.byref(ng)), "rt_build_hierarchy")
    g = int(ng.value)
    return items, bounds[:g].copy(), ranges[:g].copy(), order.astype(np.int64)


def build_hierarchy_reference(spheres, leaf_size=4, precision=capi.RT_F32, eye=None, steps=20):
    """The arithmetic of csrc/host/hierarchy.hpp restated in numpy, operation for operation (test infrastructure: slow -- a few numpy calls
    per group and per Badoiu-Clarkson step).  Same return value as build_hierarchy."""
    R = _real(precision)
    sp = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    if sp.shape[0] == 0:
        raise ValueError("build_hierarchy needs at least one sphere")
    order, bounds, ranges = [], [], []
    e = None if eye is None else np.asarray(eye, dtype=np.float64).reshape(3)

    def reach(c, r, centre):
        d = c - centre
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + r

    def enclosing(idx):
        c, r = sp[idx, :3], sp[idx, 3]
        lo, hi = (c - r[:, None]).min(axis=0), (c + r[:, None]).max(axis=0)
        centre = (lo + hi) * 0.5
        for k in range(1, steps + 1):
            if idx.size <= 1:
                break
            j = int(np.argmax(reach(c, r, centre)))            # the first of the farthest
            v = c[j] - centre
            nrm = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if nrm == 0.0:
                break
            far = c[j] + (v / nrm) * r[j]
            centre = centre + (far - centre) / float(k + 1)
        radius = float(reach(c, r, centre).max()) * (1.0 + 1e-4) + 1e-30
        return (float(centre[0]), float(centre[1]), float(centre[2]), radius)

    def build(idx, bound):
        gi = len(bounds)
        bounds.append(bound)
        ranges.append(None)
        first = len(order)
        if idx.size <= leaf_size:
            order.extend(int(i) for i in idx)
        else:
            c = sp[idx, :3]
            axis = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
            srt = idx[np.argsort(c[:, axis], kind="stable")]
            half = srt.size // 2
            parts = [srt[:half], srt[half:]]
            b = [enclosing(parts[0]), enclosing(parts[1])]
            nearer = 0
            if e is not None:
                key = []
                for k in range(2):
                    dx, dy, dz = b[k][0] - e[0], b[k][1] - e[1], b[k][2] - e[2]
                    key.append((dx * dx + dy * dy) + dz * dz)
                if key[1] < key[0]:
                    nearer = 1
            build(parts[nearer], b[nearer])
            build(parts[1 - nearer], b[1 - nearer])
        ranges[gi] = (first, len(order) - first)

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    all_idx = np.arange(sp.shape[0])
    build(all_idx, enclosing(all_idx))
    order = np.asarray(order, dtype=np.int64)
    return (sp[order].astype(R), np.asarray(bounds, dtype=np.float64).astype(R),
            np.asarray(ranges, dtype=np.int32).reshape(-1, 2), order)


class Scene:
    """Scene{group, directional_light, eye} (render.rs:138-142) with the group flattened to DFS arrays."""

    def __init__(self, items, directional_light, eye, bounds=None, ranges=None, precision=capi.RT_F32):
        R = _real(precision)
        self.precision = precision
        self.items = np.ascontiguousarray(items, dtype=R).reshape(-1, 4)
        self.directional_light = np.ascontiguousarray(directional_light, dtype=R).reshape(3)
        self.eye = np.ascontiguousarray(eye, dtype=R).reshape(3)
        self.bounds = None if bounds is None else np.ascontiguousarray(bounds, dtype=R).reshape(-1, 4)
        self.ranges = None if ranges is None else np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
        self._device = {}

    @classmethod
    def default(cls, level=8, precision=capi.RT_F32):
        """Scene::default() render.rs:144-166 (level 8 there)."""
        items, bounds, ranges = pyramid(level, (0.0, -1.0, 0.0), 1.0, precision)
        return cls(items, normalized((-1.0, -3.0, 2.0), precision), (0.0, 0.0, -4.0), bounds, ranges, precision)

    @classmethod
    def from_spheres(cls, spheres, bound, light=(-1.0, -3.0, 2.0), eye=(0.0, 0.0, -4.0), precision=capi.RT_F32):
        """One group {bound, children = spheres as Items}; BASELINE config 1's "3 spheres, 1 light" shape."""
        items = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        return cls(items, normalized(light, precision), eye, np.asarray(bound, dtype=np.float64).reshape(1, 4),
                   np.array([[0, items.shape[0]]], dtype=np.int32), precision)

    @classmethod
    def from_spheres_auto(cls, spheres, light=(-1.0, -3.0, 2.0), eye=(0.0, 0.0, -4.0), leaf_size=4, precision=capi.RT_F32):
        """Arbitrary sphere list with an automatically built bounding-sphere hierarchy (build_hierarchy)."""
        items, bounds, ranges, _ = build_hierarchy(spheres, leaf_size, precision, eye=eye)
        return cls(items, normalized(light, precision), eye, bounds, ranges, precision)

    @classmethod
    def from_spheres_balanced(cls, spheres, light=(-1.0, -3.0, 2.0), eye=(0.0, 0.0, -4.0), leaf_size=4, precision=capi.RT_F32):
        """Arbitrary sphere list, in the caller's order, under the topology of balanced_ranges and with NO bounds: for
        .device(dynamic=True) -- which refits the bounds -- followed by DeviceScene.rebuild, which puts the spheres in Morton order and is
        what makes this topology a hierarchy worth walking."""
        items = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        return cls(items, normalized(light, precision), eye, None, balanced_ranges(items.shape[0], leaf_size), precision)

    @classmethod
    def three_spheres(cls, precision=capi.RT_F32):
        """The build-defined config-1 scene."""
        return cls.from_spheres([(0.0, -1.0, 0.0, 1.0), (-1.2, 0.2, 0.0, 0.5), (1.2, 0.2, 0.0, 0.5)],
                                (0.0, -1.0, 0.0, 3.0), precision=precision)

    def device(self, device=0, dynamic=False):
        """Uploads once per device and caches the handle (replaces Arc<Scene> sharing, render.rs:279).  dynamic=True: a scene whose spheres
        DeviceScene.update replaces in place (rt_scene_create_dynamic; bounds=None with ranges: refit from the items), served by the
        ray queries, trace and render_camera*; its own handle, cached apart from the immutable one."""
        key = (device, True) if dynamic else device
        if key not in self._device:
            self._device[key] = DeviceScene(self, device, dynamic)
        return self._device[key]


class DeviceScene:
    """Owns an rt_scene* (device copies of a Scene)."""

    def __init__(self, scene, device=0, dynamic=False):
        self.scene = scene
        self.device = device
        self.dynamic = bool(dynamic)
        h = C.c_void_p()
        nb = 0 if scene.bounds is None else scene.bounds.shape[0]
        if not dynamic:
            st = capi.lib.rt_scene_create(
                device, scene.precision, scene.items.ctypes.data, scene.items.shape[0],
                scene.directional_light.ctypes.data, scene.eye.ctypes.data,
                scene.bounds.ctypes.data if nb else None, scene.ranges.ctypes.data if nb else None, nb, C.byref(h))
            capi.check(st, "rt_scene_create")
        else:
            # a dynamic scene may have ranges and no bounds: they are refit from the items
            ng = 0 if scene.ranges is None else scene.ranges.shape[0]
            if nb and nb != ng:
                raise ValueError("bounds and ranges must have the same number of rows")
            st = capi.lib.rt_scene_create_dynamic(
                device, scene.precision, scene.items.ctypes.data, scene.items.shape[0],
                scene.directional_light.ctypes.data, scene.eye.ctypes.data,
                scene.bounds.ctypes.data if nb else None, scene.ranges.ctypes.data if ng else None, ng, C.byref(h))
            capi.check(st, "rt_scene_create_dynamic")
        self._h = h
        self._n_bounds = nb if not dynamic else (0 if scene.ranges is None else scene.ranges.shape[0])

    def update(self, items, bounds=None, stream=None, live=None):
        """rt_scene_update / rt_scene_update_device: new values for every sphere of a dynamic scene (n x 4, the scene's REAL dtype, the same
        DFS order) and, optionally, for every bound (g x 4); bounds=None refits them on the device (refit_bounds is the rule).  numpy arrays
        go through the host entry, which returns when the new scene is in place.  A torch tensor on this scene's device -- or a raw device
        pointer as int -- goes through the device entry, enqueued on `stream` (a torch stream or a hipStream_t as int; default the
        current torch stream) with the stream discipline of intersect(): queries on that stream see the new scene, other streams are the
        caller's to order.  live (rt_scene_update_live*; n values, nonzero = live, memory of the same kind as `items`; None: every slot
        live): a dead slot's sphere is never hit and takes no part in the refit, whatever bits it holds; a group without a live item
        culls for every ray and reports the bound {0, 0, 0, 0}."""
        R = _real(self.scene.precision)
        n, g = self.scene.items.shape[0], self._n_bounds
        torch = sys.modules.get("torch")
        is_t = lambda x: torch is not None and isinstance(x, torch.Tensor)
        if is_t(items) or isinstance(items, int):
            if bounds is not None and not (is_t(bounds) or isinstance(bounds, int)):
                raise ValueError("bounds must be device memory too (a tensor or a pointer), or None")
            if live is not None and not (is_t(live) or isinstance(live, int)):
                raise ValueError("live must be device memory too (a uint8 / bool tensor or a pointer), or None")
            if torch is None:
                import torch
            tdt = torch.float32 if R == np.float32 else torch.float64
            dev = torch.device("cuda", self.device)
            for x, rows, what in ((items, n, "items"), (bounds, g, "bounds")):
                if is_t(x) and (x.dtype != tdt or x.device != dev or x.numel() != 4 * rows):
                    raise ValueError("%s must be a (%d, 4) %s tensor on %s" % (what, rows, tdt, dev))
            if is_t(live) and (live.dtype not in (torch.uint8, torch.bool) or live.device != dev or live.numel() != n):
                raise ValueError("live must be a (%d,) uint8 or bool tensor on %s" % (n, dev))
            with self._stream_scope(torch, stream, (items, bounds, live)) as tail:
                it, bd, lv = (x.contiguous() if is_t(x) else x for x in (items, bounds, live))
                ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr() if is_t(x) else x)
                if lv is None:
                    rc = capi.lib.rt_scene_update_device(self._h, ptr(it), ptr(bd), *tail)
                else:
                    rc = capi.lib.rt_scene_update_live_device(self._h, ptr(it), ptr(bd), ptr(lv), *tail)
            capi.check(rc, "rt_scene_update_device" if lv is None else "rt_scene_update_live_device")
            return
        it = np.asarray(items)
        if it.dtype != R or it.size != 4 * n:
            raise ValueError("items must be a (%d, 4) array of %s" % (n, np.dtype(R).name))
        it = np.ascontiguousarray(it)
        bd = None
        if bounds is not None:
            bd = np.asarray(bounds)
            if bd.dtype != R or bd.size != 4 * g:
                raise ValueError("bounds must be a (%d, 4) array of %s" % (g, np.dtype(R).name))
            bd = np.ascontiguousarray(bd)
        bdp = None if bd is None or g == 0 else bd.ctypes.data
        if live is None:
            capi.check(capi.lib.rt_scene_update(self._h, it.ctypes.data, bdp), "rt_scene_update")
            return
        lv = np.asarray(live)
        if lv.dtype not in (np.uint8, np.bool_) or lv.size != n:
            raise ValueError("live must be a (%d,) array of uint8 or bool" % n)
        lv = np.ascontiguousarray(lv).view(np.uint8)
        capi.check(capi.lib.rt_scene_update_live(self._h, it.ctypes.data, bdp, lv.ctypes.data), "rt_scene_update_live")

    def _device_stream(self, torch, stream):
        """(the torch stream a device entry is enqueued on, the current one) for `stream`: None, a torch stream or a hipStream_t as int."""
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(dev)
        if stream is None:
            return cur, cur
        if isinstance(stream, torch.cuda.Stream):
            return stream, cur
        hs = int(stream)
        return (torch.cuda.default_stream(dev) if hs == 0 else torch.cuda.ExternalStream(hs, device=dev)), cur

    @contextlib.contextmanager
    def _stream_scope(self, torch, stream, tensors):
        """The scope a device entry is called in -> the entry's stream argument, as a 1-tuple.  The call runs on `qs`, the stream `stream`
        names.  It first waits for what the caller has queued on the current stream (the inputs were made there), and everything
        allocated inside the scope -- copies of the inputs, the results -- comes from qs's pool, so no allocation of another stream can
        reuse that memory while the call still uses it.  The caller's own tensors among `tensors`, inputs and outputs alike, are marked
        as used on qs when the scope is left."""
        qs, cur = self._device_stream(torch, stream)
        if qs != cur:
            qs.wait_stream(cur)
        with torch.cuda.stream(qs):
            yield (qs.cuda_stream,)
        if qs != cur:
            for x in tensors:
                if isinstance(x, torch.Tensor) and x.is_cuda:
                    x.record_stream(qs)

    def _side(self, x=None, device=False):
        """The argument side of a call: the device side for a torch tensor `x` (or device=True), the host side otherwise."""
        torch = sys.modules.get("torch")
        if not device and (torch is None or not isinstance(x, torch.Tensor)):
            return _HOST_SIDES[self.scene.precision]
        key = (self.scene.precision, self.device)
        side = _DEVICE_SIDES.get(key)
        if side is None:
            import torch
            side = _DEVICE_SIDES[key] = _DeviceSide(torch, _real(self.scene.precision), self.device)
        return side

    def _order_query(self, entry, x, name, cols, rows, stream, n=None, with_n=True):
        """The body of ray_order, sphere_order and the rebuilds: entry(scene, x[, n], order_out[, stream]) -> uint32[n].  n: None -- every
        row of x; else that many of them (0: nothing is read or written, and x may be empty)."""
        side = self._side(x)
        with side.scope(self, stream, (x,)) as tail:
            if not (n == 0 and x.shape[0] == 0):
                x = side.real_rows(x, name, cols, rows)
            m = x.shape[0] if n is None else n
            order = side.empty((m,), np.uint32)
            args = (side.ptr(x) if m else None,) + ((m,) if with_n else ()) + (side.ptr(order) if m else None,)
            rc = getattr(capi.lib, entry + side.suffix)(self._h, *args, *tail)
        capi.check(rc, entry + side.suffix)
        return order

    def sphere_order(self, spheres, stream=None):
        """rt_sphere_order / rt_sphere_order_device: the Morton order of `spheres` (n x 4, the scene's REAL dtype; any n), computed on the
        device -> uint32[n]: np.argsort(sphere_keys(spheres), kind="stable").  numpy in, numpy out; a torch tensor on this scene's device goes
        through the device entry on `stream` (as ray_order routes) and gives a torch.uint32 tensor."""
        return self._order_query("rt_sphere_order", spheres, "spheres", 4, None, stream)

    def rebuild(self, spheres, stream=None, n=None):
        """rt_scene_rebuild / rt_scene_rebuild_device: the hierarchy of a dynamic scene rebuilt from `spheres` (n_items x 4, the scene's REAL
        dtype) in ANY order -> the order, uint32[n_items]: DFS slot k now holds spheres[order[k]] (what a query's item index names), every
        bound is refit, and the scene answers as a fresh one made from spheres[order], bounds() and the same ranges.  order is
        np.argsort(sphere_keys(spheres), kind="stable").  numpy goes through the host entry, which returns when the new scene is in place;
        a torch tensor on this scene's device goes through the device entry, enqueued on `stream` with the discipline of update().
        n (rt_scene_rebuild_n*; None: all n_items): the first n rows of `spheres`, 0 <= n <= n_items, into slots 0 .. n-1 in their own
        sphere order -> uint32[n]; every slot from n on is dead, n = 0 empties the scene."""
        cap = self.scene.items.shape[0]
        if n is None:
            return self._order_query("rt_scene_rebuild", spheres, "spheres", 4, cap, stream, with_n=False)
        n = int(n)
        if not 0 <= n <= cap:
            raise capi.RtError(capi.RT_ERR_INVALID_ARGUMENT, "rt_scene_rebuild_n", "n = %d is outside 0 .. %d, the scene's capacity" % (n, cap))
        if not (hasattr(spheres, "shape") and len(spheres.shape) == 2 and n <= spheres.shape[0]):
            raise ValueError("rebuild: spheres must have at least n = %d rows" % n)
        return self._order_query("rt_scene_rebuild_n", spheres, "spheres", 4, None, stream, n=n)

    def live(self):
        """rt_scene_live -> uint8[n_items] of 0 / 1: which slots are live (after the last update or rebuild; an immutable scene: all ones)."""
        out = np.zeros(self.scene.items.shape[0], dtype=np.uint8)
        capi.check(capi.lib.rt_scene_live(self._h, out.ctypes.data), "rt_scene_live")
        return out

    def bounds(self):
        """rt_scene_bounds -> REAL[g, 4]: the scene's current bounds (after the last update; an immutable scene: as created)."""
        out = np.zeros((self._n_bounds, 4), dtype=_real(self.scene.precision))
        capi.check(capi.lib.rt_scene_bounds(self._h, out.ctypes.data if self._n_bounds else None), "rt_scene_bounds")
        return out

    def traits(self):
        """rt_scene_traits -> bit set of capi.RT_SCENE_HAS_BOUNDS / capi.RT_SCENE_CONCENTRIC."""
        t = C.c_uint32(0)
        capi.check(capi.lib.rt_scene_traits(self._h, C.byref(t)), "rt_scene_traits")
        return t.value

    def setup_cost(self):
        """rt_scene_setup_cost -> (total_ms, stream_ms) of the rt_scene_create call that made this scene."""
        total, stream = C.c_double(0), C.c_double(0)
        capi.check(capi.lib.rt_scene_setup_cost(self._h, C.byref(total), C.byref(stream)), "rt_scene_setup_cost")
        return total.value, stream.value

    def close(self):
        if getattr(self, "_h", None):
            capi.lib.rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _regions(regions):
        arr = (capi.Region * len(regions))()
        for i, (l, t, r, b) in enumerate(regions):
            arr[i] = capi.Region(l, t, r, b)
        return arr

    def render_tiles(self, options, regions, traversal=None, want_stats=True, out=None):
        """rt_render_tiles: regions = [(l, t, r, b), ...] -> (uint8[total_px*4] tile-major, stats dict | None).
        out: optional uint8 array to render into.  Pinned memory is written by the kernel directly: keep the allocation in a
        variable while its array is in use -- `hb = capi.HostBuffer(n); dev.render_tiles(..., out=hb.array)`."""
        traversal = self.default_traversal() if traversal is None else traversal
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        nbytes = capi.lib.rt_tiles_rgba_bytes(arr, len(arr))
        if out is None:
            out = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < nbytes:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % nbytes)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_tiles(self._h, C.byref(o), traversal, arr, len(arr), out.ctypes.data,
                                      C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_tiles")
        return out.reshape(-1)[:int(nbytes)], (st.as_dict() if want_stats else None)

    def render_region(self, options, region, traversal=None, want_stats=False, out=None):
        """rt_render_region: one bucket (l, t, r, b) -> (uint8[h, w, 4], stats dict | None); the literal render.rs:283-294 call."""
        traversal = self.default_traversal() if traversal is None else traversal
        l, t, r, b = region
        reg = capi.Region(l, t, r, b)
        nbytes = (t - b) * (r - l) * 4
        if out is None:
            out = np.empty(nbytes, dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < nbytes:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % nbytes)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_region(self._h, C.byref(o), traversal, C.byref(reg), out.ctypes.data, C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_region")
        return out.reshape(-1)[:nbytes].reshape(t - b, r - l, 4), (st.as_dict() if want_stats else None)

    def render_tiles_stream(self, options, regions, on_tile, traversal=None):
        """rt_render_tiles_stream: on_tile(index, (l, t, r, b), uint8[h, w, 4] view valid during the call) for every bucket, in
        completion order, while later batches are still rendering (the reference's channel consumer, render.rs:301-307)."""
        traversal = self.default_traversal() if traversal is None else traversal
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        err = []

        def cb(_user, index, region, rgba):
            if err:
                return
            try:
                reg = region.contents
                h, w = reg.t - reg.b, reg.r - reg.l
                on_tile(int(index), (reg.l, reg.t, reg.r, reg.b), np.ctypeslib.as_array(rgba, shape=(h * w * 4,)).reshape(h, w, 4))
            except BaseException as e:      # noqa: BLE001  (must not unwind through the C frames)
                err.append(e)

        o = capi.Options(*options)
        rc = capi.lib.rt_render_tiles_stream(self._h, C.byref(o), traversal, arr, len(arr), capi.TILE_CALLBACK(cb), None)
        if err:
            raise err[0]
        capi.check(rc, "rt_render_tiles_stream")

    def render_frame_stream(self, options, regions, frame_format, out, on_batch=None, traversal=None):
        """rt_render_frame_stream: the listed buckets, converted on the device, into their place in `out` -- a row-major uint8 frame in
        the file's pixel format (capi.RT_FRAME_RGBA / _RGB / _GREY: 4 / 3 / 1 bytes per pixel).  on_batch(first_tile, n_tiles) after each
        batch is in place.  A capi.HostBuffer array is written by the device directly."""
        traversal = self.default_traversal() if traversal is None else traversal
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        bpp = {capi.RT_FRAME_RGBA: 4, capi.RT_FRAME_RGB: 3, capi.RT_FRAME_GREY: 1}[frame_format]
        if out.dtype != np.uint8 or out.size != options[0] * options[1] * bpp or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous uint8 array of width * height * %d bytes" % bpp)
        err = []

        def cb(_user, first, count):
            if err or on_batch is None:
                return
            try:
                on_batch(int(first), int(count))
            except BaseException as e:      # noqa: BLE001  (must not unwind through the C frames)
                err.append(e)

        o = capi.Options(*options)
        rc = capi.lib.rt_render_frame_stream(self._h, C.byref(o), traversal, arr, len(arr), frame_format, out.ctypes.data, capi.BATCH_CALLBACK(cb), None)
        if err:
            raise err[0]
        capi.check(rc, "rt_render_frame_stream")
        return out

    def default_traversal(self):
        """The reference's hierarchy walk whenever the scene has bounds; the flat scan otherwise."""
        return capi.RT_TRAVERSAL_SKIP if self.scene.bounds is not None and len(self.scene.bounds) else capi.RT_TRAVERSAL_FLAT

    def render_tiles_device(self, options, regions, out_ptr, stream=0, traversal=None, want_stats=False):
        """rt_render_tiles_device: enqueue on `stream` (hipStream_t as int), output to device pointer `out_ptr`."""
        traversal = self.default_traversal() if traversal is None else traversal
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_tiles_device(self._h, C.byref(o), traversal, arr, len(arr), C.c_void_p(out_ptr),
                                             C.c_void_p(stream), C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_tiles_device")
        return st.as_dict() if want_stats else None

    def render_frame_device(self, options, regions, frame_ptr, stream=0, traversal=capi.RT_TRAVERSAL_SKIP, want_stats=False):
        """rt_render_frame_device: the buckets rendered straight into a row-major device frame (render + blit fused)."""
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_frame_device(self._h, C.byref(o), traversal, arr, len(arr), C.c_void_p(frame_ptr),
                                             C.c_void_p(stream), C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_frame_device")
        return st.as_dict() if want_stats else None

    def _fixed_query(self, entry, x, name, cols, names, values, exclude, order, true_ok, specs, out, want_stats, stream, layout, rows=()):
        """The body of every query with one fixed-size result per query: `entry` (host side) or `entry`_device is called with the scene and
        layout(x, reals, n, exclude, order, results, stats, stream) -- pointers, or NULL for None; reals and results are lists; stream is
        () on the host side and the 1-tuple of the stream on the device side -- and the results come back as a tuple[, stats dict].
        x: the main input, `name`, n x cols of the scene's REAL, whose memory kind chooses the side.  names, values: the per-query reals,
        each one value, (n,) REAL or None.  rows: further inputs with rows of REAL, each (array, name, cols, _N or _ITEMS, optional) as
        _list_query takes them; their pointers follow the per-query reals' in `reals`.  exclude: int32[n] or None.  order: None or
        uint32[n]; True passes as NULL where true_ok.  specs: (shape behind n, dtype) of each result, "R" for the scene's REAL; out: such
        arrays or tensors to fill, or None."""
        side = self._side(x)
        st = capi.Stats()
        stp = C.byref(st) if want_stats else None
        with side.scope(self, stream, (x, exclude, order, *values, *[r[0] for r in rows], *(() if out is None else out))) as tail:
            x = side.real_rows(x, name, cols)
            n = x.shape[0]
            reals = [side.per_query(v, what, n) for what, v in zip(names, values)]
            reals += [side.real_rows(y, what, c, n if count is _N else self.scene.items.shape[0], optional) for y, what, c, count, optional in rows]
            ex = side.exclude(exclude, n)
            o = None if order is None or (order is True and true_ok) else side.order(order, n)
            if out is None:
                res = tuple([side.empty((n,) + shape, dt) for shape, dt in specs])
            else:
                res = side.check_out(out, [((n,) + shape, dt) for shape, dt in specs])
            ptr = side.ptr
            rc = getattr(capi.lib, entry + side.suffix)(
                self._h, *layout(ptr(x), [ptr(r) for r in reals], n, ptr(ex), ptr(o), [ptr(a) for a in res], stp, tail))
        capi.check(rc, entry + side.suffix)
        return res + (st.as_dict(),) if want_stats else res

    def _ray_query(self, entry, head, rays, values, order, specs, out, want_stats, stream):
        """_fixed_query for the ray entries: entry(scene, *head, rays[, tmax], n, results...[, stream], stats), which with an order (True or
        indices) is `entry`_ordered, whose order pointer follows n.  values: (tmax,) or ().  Known gap: with tensors `out` is ignored."""
        ordered = order is not None
        return self._fixed_query(entry + "_ordered" if ordered else entry, rays, "rays", 6, ("tmax",), values, None, order, True, specs,
                                 out if isinstance(rays, np.ndarray) else None, want_stats, stream,
                                 lambda x, t, n, ex, o, res, stats, stream: (*head, x, *t, n, *((o,) if ordered else ()), *res, *stream, stats))

    def _list_query(self, entry, side, xs, shapes, exclude, order, capacity, wanted, columns, offsets, stats, stream, what, head):
        """The body of every query that lists: `entry` + side.suffix is called with the scene, head(inputs, n, exclude, order) -- pointers, or
        NULL for None -- and then capacity, a pointer per column, offsets, total, stats[, stream]; -> (columns..., [offsets,] total[, stats
        dict]).  xs: the inputs, each with its (name, cols, rows, optional) in shapes for side.real_rows -- rows None: any n > 0, which
        exclude, order and the offsets then go by; _N: n rows; _ITEMS: one per item of the scene (without an n the offsets go by the
        items too).  order=True: the sphere order of the first input with unit radii, on the same stream.  capacity=None: a counting call
        first, then exactly that many entries (`what` % count names them when there are too many).  columns: (shape behind the entry
        count, dtype) each, made where `wanted`.  The host side trims the columns to min(capacity, total) and gives total as an int; the
        device side waits for nothing unless it had to count: total is then a 0-d int64 tensor."""
        if capacity is not None:
            capacity = int(capacity)
            if not 0 <= capacity <= 0x7FFFFFFF:
                raise ValueError("capacity must be None or 0 .. 2^31 - 1, not %d" % capacity)
        st = capi.Stats()
        stp = C.byref(st) if stats else None
        ptr = side.ptr
        with side.scope(self, stream, (*xs, exclude, order)) as tail:
            n, n_items, staged, ptrs = None, self.scene.items.shape[0], [], []
            for x, (name, cols, rows, optional) in zip(xs, shapes):
                x = side.real_rows(x, name, cols, n if rows is _N else n_items if rows is _ITEMS else None, optional)
                if rows is None:
                    n = x.shape[0]
                staged.append(x)
                ptrs.append(ptr(x))
            ex = side.exclude(exclude, n)
            if order is True:
                unit = side.copy(staged[0])
                unit[:, 3] = 1                                                   # (the radii take no part in the order, and q = 0 is no sphere)
                o = self.sphere_order(unit)                                      # (on the scope's stream: it is the current one)
            else:
                o = None if order is None else side.order(order, n)
            total, totp = side.total_cell()
            off = side.empty(((n_items if n is None else n) + 1,), np.uint64) if offsets else None
            f = getattr(capi.lib, entry + side.suffix)
            args = head(ptrs, n, ptr(ex), ptr(o))
            counted = capacity is None
            if counted:
                capi.check(f(self._h, *args, 0, *[None] * len(columns), None, totp, None, *tail), entry + side.suffix)
                capacity = side.read_total(total)
                if capacity > 0x7FFFFFFF:
                    raise ValueError("%s, more than one call can list: pass a capacity" % (what % capacity))
            listed = [side.empty((capacity,) + shape, dt) if w else None for w, (shape, dt) in zip(wanted, columns)]
            rc = f(self._h, *args, capacity, *[ptr(c) if capacity else None for c in listed], ptr(off), totp, stp, *tail)
        capi.check(rc, entry + side.suffix)
        if side.trims or counted:
            total = side.read_total(total)
        m = min(capacity, total) if side.trims else None
        res = [c if m is None else c[:m] for c in listed if c is not None]
        if offsets:
            res.append(off)
        res.append(total)
        if stats:
            res.append(st.as_dict())
        return tuple(res)


    def intersect(self, rays, tmax=None, any_hit=False, want_stats=False, stream=None, out=None, order=None):
        """rt_intersect_rays / rt_intersect_rays_device: TypedGroup::intersect for every ray of `rays` (n x 6: pos.xyz, dir.xyz, the scene's REAL
        dtype) -> (distance[n], normal[n, 3], item[n] (DFS index or -1)[, stats dict]).  tmax: hit.distance going in, per ray (an array of
        the scene's REAL) or one value (rounded to REAL; None: +inf).  any_hit: occlusion -- the first item closer than tmax instead of the nearest.
        A numpy array goes through the host entry and gets numpy results (out: optional (distance, normal, item) arrays to fill, e.g. from
        capi.HostBuffer, which the kernel then writes directly); a torch tensor on this scene's device goes through the device entry on
        `stream` (a torch stream or a hipStream_t as int; default the current torch stream) and gets torch tensors on that device: the
        query waits for the work queued on the current torch stream, and its results belong to `stream` (use them there, or synchronise).
        order (rt_intersect_rays_ordered*): None -- the rays are walked as they are stored; True -- the call orders them on the device first
        (ray_order) and walks in that order; or an index array / tensor (uint32[n], a permutation: lane j carries ray order[j]).  The results
        and counters are the same bytes whatever the order; only the time differs."""
        mode = capi.RT_QUERY_ANY if any_hit else capi.RT_QUERY_NEAREST
        return self._ray_query("rt_intersect_rays", (mode,), rays, (tmax,), order, (((), "R"), ((3,), "R"), ((), np.int32)), out, want_stats, stream)

    def intersect_multi(self, rays, k, tmax=None, all_hits=False, want_stats=False, stream=None, out=None, order=None):
        """rt_intersect_rays_multi / rt_intersect_rays_multi_device: the k closest hits of every ray, nearest first, equal distances in DFS
        order -> (distance[n, k], normal[n, k, 3], item[n, k] (DFS index or -1), hits[n] (uint32)[, stats dict]).  An empty slot reads tmax,
        -1 and (0, 0, 0).  all_hits=False (RT_MULTIHIT_CLOSEST): hits = the filled slots; with k = 1 this is intersect() exactly.
        all_hits=True (RT_MULTIHIT_ALL): no culling below tmax, hits = every item below tmax (may exceed k), the list its k closest.
        1 <= k <= RT_MULTIHIT_MAX_K.  rays, tmax, stream, order and out (here (distance, normal, item, hits)) as for intersect()."""
        k = int(k)
        if not 1 <= k <= capi.RT_MULTIHIT_MAX_K:
            raise ValueError("k must be 1 .. %d, not %d" % (capi.RT_MULTIHIT_MAX_K, k))
        mode = capi.RT_MULTIHIT_ALL if all_hits else capi.RT_MULTIHIT_CLOSEST
        return self._ray_query("rt_intersect_rays_multi", (mode, k), rays, (tmax,), order,
                               (((k,), "R"), ((k, 3), "R"), ((k,), np.int32), ((), np.uint32)), out, want_stats, stream)

    def near(self, points, k, radius=None, all_within=False, exclude=None, want_stats=False, stream=None, out=None, order=None):
        """rt_near_spheres / rt_near_spheres_device: the k nearest spheres of every point of `points` (n x 3, the scene's REAL dtype), by
        surface gap (sphere_gaps is the metric: negative inside a sphere), nearest first, equal gaps in DFS order -> (gap[n, k], item[n, k]
        (DFS slot or -1), found[n] (uint32)[, stats dict]).  radius: the search radius per point (an array of the scene's REAL) or one value
        (rounded to REAL; None: +inf); only spheres with a gap below it are listed, and an empty slot reads the radius and -1.
        all_within=False (RT_NEAR_CLOSEST): found = the filled slots.  all_within=True (RT_NEAR_ALL): found = every sphere below the
        radius (may exceed k), the list its k nearest.  1 <= k <= RT_NEAR_MAX_K.  exclude (int32[n]): the item slot each query ignores --
        np.arange(n) for the self-queries of the scene's own items; -1 or a slot outside the scene excludes nothing.  A dead slot of a
        dynamic scene is never listed.  numpy arrays go through the host entry, a torch tensor on this scene's device through the device
        entry on `stream`, with the stream discipline of intersect(); out: optional (gap, item, found) arrays / tensors to fill.
        order (uint32[n]): lane j carries query order[j]; the results and counters are the same bytes whatever the order, only the time
        differs.  The host entry wants a permutation; through the device entry an index >= n carries no query and leaves that thread's
        outputs alone.  A query is a sphere-shaped record, so a coherent order is
            order = dev.sphere_order(np.concatenate([points, np.ones((n, 1), points.dtype)], axis=1))."""
        k = int(k)
        if not 1 <= k <= capi.RT_NEAR_MAX_K:
            raise ValueError("k must be 1 .. %d, not %d" % (capi.RT_NEAR_MAX_K, k))
        mode = capi.RT_NEAR_ALL if all_within else capi.RT_NEAR_CLOSEST
        return self._fixed_query("rt_near_spheres", points, "points", 3, ("radius",), (radius,), exclude, order, False,
                                 (((k,), "R"), ((k,), np.int32), ((), np.uint32)), out, want_stats, stream,
                                 lambda p, r, n, ex, o, res, stats, stream: (mode, k, p, r[0], n, ex, o, *res, stats, *stream))

    def sweep(self, rays, radius=None, tmax=None, any_hit=False, exclude=None, order=None, want_stats=False, stream=None, out=None):
        """rt_sweep_spheres / rt_sweep_spheres_device: the first contact of a moving sphere with the scene, for every cast of `rays` (n x 6:
        pos.xyz, dir.xyz with dir a unit vector, the scene's REAL dtype) -> (distance[n], normal[n, 3], item[n] (DFS slot or -1)[, stats
        dict]).  radius: the moving sphere's radius per cast (an array of the scene's REAL) or one value (rounded to REAL; None: 0, a ray);
        tmax: the cutoff per cast, likewise (None: +inf).  sweep_distances is the metric: the distance the centre travels until the
        moving sphere touches a sphere of the scene, 0 when it touches or overlaps one at its start.  A cast without a contact below tmax
        reads tmax, a zero normal and -1.  any_hit=False (RT_SWEEP_NEAREST): the first contact, equal distances to the first item in DFS
        order.  any_hit=True (RT_SWEEP_ANY): some contact below tmax, found sooner.  exclude (int32[n]): the item slot each cast ignores --
        np.arange(n) when the scene's own items are cast from their own poses; -1 or a slot outside the scene excludes nothing.  A dead
        slot of a dynamic scene is never returned.  numpy arrays go through the host entry, a torch tensor on this scene's device through
        the device entry on `stream`, with the stream discipline of intersect(); out: optional (distance, normal, item) arrays / tensors
        to fill.  order (uint32[n]): lane j carries cast order[j]; the results and counters are the same bytes whatever the order, only
        the time differs.  The host entry wants a permutation; through the device entry an index >= n carries no cast and leaves that
        thread's outputs alone."""
        mode = capi.RT_SWEEP_ANY if any_hit else capi.RT_SWEEP_NEAREST
        return self._fixed_query("rt_sweep_spheres", rays, "rays", 6, ("radius", "tmax"), (radius, tmax), exclude, order, False,
                                 (((), "R"), ((3,), "R"), ((), np.int32)), out, want_stats, stream,
                                 lambda y, qt, n, ex, o, res, stats, stream: (mode, y, qt[0], qt[1], n, ex, o, *res, stats, *stream))

    def contacts(self, margin=0.0, capacity=None, gaps=False, offsets=False, stats=False, device=False, stream=None):
        """rt_scene_contacts / rt_scene_contacts_device: every pair of spheres of the scene that is closer than `margin` (pair_gaps is the
        metric; 0: the overlapping spheres, a positive margin is a skin, a negative one asks for that much overlap, +inf gives every pair
        of live spheres) -> (pairs[, gap][, offsets], total[, stats dict]).  pairs: int32[m, 2], the DFS slots i < j of every contact,
        sorted by (i, j), the same bytes every time; a dead slot of a dynamic scene is in no pair.  gaps=True: REAL[m], each pair's gap.
        offsets=True: uint64[n_items + 1], item i is the lower slot of pairs offsets[i] .. offsets[i + 1].  total: how many pairs there
        are.  capacity=None counts first and then allocates exactly (m = total); with a capacity, m = min(capacity, total) and the list is
        the exact prefix of the full one; capacity=0 only counts.  device=False: the host entry, numpy results.  device=True: the device
        entry on `stream` (a torch stream or a hipStream_t as int; default the current torch stream), torch tensors on the scene's device
        -- with a capacity nothing is waited for: pairs has `capacity` rows of which the first `total` are written, and total is a 0-d
        int64 tensor (offsets is an int64 tensor too: the same bits); capacity=None reads the count back first, and total is an int."""
        margin = float(margin)
        if margin != margin:
            raise ValueError("margin must not be NaN")
        return self._list_query("rt_scene_contacts", self._side(device=device), (), (), None, None, capacity, (True, gaps), (((2,), np.int32), ((), "R")),
                                offsets, stats, stream, "the scene has %d contacts", lambda xs, n, ex, o: (margin,))

    def overlaps(self, queries, margin=0.0, exclude=None, order=None, capacity=None, gaps=False, offsets=False, stats=False, stream=None):
        """rt_overlap_spheres / rt_overlap_spheres_device: every sphere of the scene within `margin` of each query sphere of `queries`
        (n x 4: px, py, pz, q, the scene's REAL dtype -- the layout of a sphere array; overlap_gaps is the metric; margin 0: the spheres a
        query overlaps, a positive margin is a skin, a negative one asks for that much overlap, +inf lists every live sphere) ->
        (items[, gap][, offsets], total[, stats dict]).  items: int32[m], the DFS slots of the listed spheres, query after query, ascending
        within a query, the same bytes every time; a dead slot of a dynamic scene is never listed.  gaps=True: REAL[m], each entry's gap.
        offsets=True: uint64[n + 1], query g owns entries offsets[g] .. offsets[g + 1].  total: how many entries there are.
        capacity=None counts first and then allocates exactly (m = total); with a capacity, m = min(capacity, total) and the list is the
        exact prefix of the full one; capacity=0 only counts.  exclude (int32[n]): the item slot each query never lists (-1 or a slot
        outside the scene: none).  order (uint32[n]): thread j carries query order[j] -- the same bytes and counters in every order; True
        asks sphere_order for a coherent one (by centre).  numpy arrays go through the host entry and give numpy results.  A torch
        tensor on this scene's device goes through the device entry on `stream` (a torch stream or a hipStream_t as int; default the current
        torch stream) and gives torch tensors -- with a capacity nothing is waited for: items has `capacity` entries of which the first
        `total` are written, and total is a 0-d int64 tensor (offsets is an int64 tensor too: the same bits); capacity=None reads the
        count back first, and total is an int.  Through the device entry an order entry >= n carries no query, and a query that no
        thread carries, or whose q is not >= 0, has an empty row."""
        margin = float(margin)
        if margin != margin:
            raise ValueError("margin must not be NaN")
        return self._list_query("rt_overlap_spheres", self._side(queries), (queries,), (("queries", 4, None, False),), exclude, order, capacity,
                                (True, gaps), (((), np.int32), ((), "R")), offsets, stats, stream, "the queries have %d entries",
                                lambda xs, n, ex, o: (xs[0], n, margin, ex, o))

    def box_overlaps(self, boxes, margin=0.0, exclude=None, order=None, capacity=None, gaps=False, offsets=False, stats=False, stream=None):
        """rt_overlap_boxes / rt_overlap_boxes_device: every sphere of the scene within `margin` of each axis-aligned box of `boxes` (n x 6:
        lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, the scene's REAL dtype; box_gaps is the metric: the distance from the box to the sphere's
        surface, -r for a centre inside the box; margin 0: the spheres a box touches, a positive margin is a skin, +inf lists every live
        sphere) -> (items[, gap][, offsets], total[, stats dict]), with the shapes, capacity, exclude, stream and the host / device routing
        of overlaps().  A side may be infinite (a slab, a half-space); lo == hi is a point.  The host entry refuses a NaN coordinate and
        an inverted box (lo > hi on some axis); through the device entry such a box carries no query and has an empty row.
        order (uint32[n]): thread j carries box order[j] -- the same bytes and counters in every order.  order=True is refused: there is
        no sphere array to order by.  For finite boxes a coherent order is the sphere order of their centres with radius 1:
            centres = 0.5 * (boxes[:, :3] + boxes[:, 3:])
            order = dev.sphere_order(np.concatenate([centres, np.ones((n, 1), boxes.dtype)], axis=1))."""
        margin = float(margin)
        if margin != margin:
            raise ValueError("margin must not be NaN")
        if order is True:
            raise ValueError("order=True is not available for boxes: pass sphere_order of the boxes' centres with radius 1")
        return self._list_query("rt_overlap_boxes", self._side(boxes), (boxes,), (("boxes", 6, None, False),), exclude, order, capacity,
                                (True, gaps), (((), np.int32), ((), "R")), offsets, stats, stream, "the boxes have %d entries",
                                lambda xs, n, ex, o: (xs[0], n, margin, ex, o))

    def region_overlaps(self, planes, margin=0.0, sections=None, capacity=None, gaps=False, offsets=False, stats=False, stream=None):
        """rt_overlap_regions / rt_overlap_regions_device: every sphere of the scene that reaches into each convex region of `planes`
        (n x 6 x 4 or n x 24, the scene's REAL dtype: six planes {n.x, n.y, n.z, d} with unit normals, outside where n.c + d > 0, an absent
        plane (0, 0, 0, -inf); region_gaps is the metric: the largest signed plane distance of the centre minus the radius, so the list is
        a superset of the exact touch list; camera_planes and box_planes make such regions) -> (items[, gap][, offsets], total[, stats
        dict]), with the shapes, capacity, stream and the host / device routing of overlaps().  The call is made for FEW regions that
        each cover much of the scene: a wave carries one region and its lanes sections of the node stream.  sections (None or 0: the
        library's rule, region_sections(n, n_nodes)): how many sections a region is cut into -- the list is the same bytes for every
        value, only the time and the test counters differ.  The host entry refuses a NaN in a plane and a normal that is not of
        length 1; through the device entry a region with a NaN carries no query and has an empty row."""
        margin = float(margin)
        if margin != margin:
            raise ValueError("margin must not be NaN")
        sections = 0 if sections is None else int(sections)
        if not 0 <= sections <= 0xFFFFFFFF:
            raise ValueError("sections must be None or 0 .. 2^32 - 1, not %d" % sections)
        if getattr(planes, "ndim", None) == 3 and tuple(planes.shape[1:]) == (6, 4):
            planes = planes.reshape(planes.shape[0], 24)
        return self._list_query("rt_overlap_regions", self._side(planes), (planes,), (("planes", 24, None, False),), None, None, capacity,
                                (True, gaps), (((), np.int32), ((), "R")), offsets, stats, stream, "the regions have %d entries",
                                lambda xs, n, ex, o: (xs[0], n, margin, sections))

    def impacts(self, disp, capacity=None, times=False, offsets=False, stats=False, stream=None):
        """rt_scene_impacts / rt_scene_impacts_device: every pair of spheres of the scene that comes into contact while sphere k moves from
        c_k to c_k + disp[k] (`disp`: n_items x 3, the scene's REAL dtype, one row per item slot -- on a live scene per slot of the capacity;
        a dead slot's row is not used; pair_impacts is the metric) -> (pairs[, time][, offsets], total[, stats dict]).  pairs: int32[m, 2],
        the DFS slots i < j of every impact, sorted by (i, j), the same bytes every time.  times=True: REAL[m], each pair's t in [0, 1] (0:
        in contact at the start).  offsets=True: uint64[n_items + 1], item i is the lower slot of pairs offsets[i] .. offsets[i + 1].
        capacity=None counts first and then allocates exactly (m = total); with a capacity, m = min(capacity, total) and the list is the
        exact prefix of the full one; capacity=0 only counts (times needs pairs: times=True with capacity=0 is an error).  A numpy array
        goes through the host entry and gives numpy results; its components must be finite and within +-1e15.  A torch tensor on this
        scene's device goes through the device entry on `stream` (a torch stream or a hipStream_t as int; default the current torch
        stream) and gives torch tensors -- with a capacity nothing is waited for: pairs has `capacity` rows of which the first `total` are
        written, and total is a 0-d int64 tensor (offsets is an int64 tensor too: the same bits); capacity=None reads the count back
        first, and total is an int."""
        if times and capacity is not None and int(capacity) == 0:
            raise ValueError("times needs pairs: capacity must not be 0")
        return self._list_query("rt_scene_impacts", self._side(disp), (disp,), (("disp", 3, _ITEMS, False),), None, None, capacity,
                                (True, times), (((2,), np.int32), ((), "R")), offsets, stats, stream, "the step has %d impacts",
                                lambda xs, n, ex, o: (xs[0],))

    def _islands_query(self, entry, side, moving, disp, head, index, sizes, stats, stream):
        """The body of islands and impact_islands: `entry` + side.suffix is called with the scene, head(disp pointer; moving: the impact
        form, which takes one) and then label, index or NULL, size or NULL, n_islands, stats[, stream]; -> (label[, index][, size],
        n_islands[, stats dict]).  The host side gives n_islands as an int; the device side waits for nothing: it is a 0-d int64 tensor."""
        st = capi.Stats()
        stp = C.byref(st) if stats else None
        ptr = side.ptr
        with side.scope(self, stream, (disp,)) as tail:
            n_items = self.scene.items.shape[0]
            d = side.real_rows(disp, "disp", 3, n_items) if moving else None
            label = side.empty((n_items,), np.int32)
            idx = side.empty((n_items,), np.int32) if index else None
            size = side.empty((n_items,), np.uint32) if sizes else None
            total, totp = side.total_cell()
            rc = getattr(capi.lib, entry + side.suffix)(self._h, *head(ptr(d)), ptr(label), ptr(idx), ptr(size), totp, stp, *tail)
        capi.check(rc, entry + side.suffix)
        res = [x for x in (label, idx, size) if x is not None]
        res.append(side.read_total(total) if side.trims else total)
        if stats:
            res.append(st.as_dict())
        return tuple(res)

    def islands(self, margin=0.0, index=False, sizes=False, stats=False, device=False, stream=None):
        """rt_scene_islands / rt_scene_islands_device: the connected groups of the scene's contacts at `margin` -- the graph on the live
        slots whose edges are the pairs contacts(margin) lists (pair_islands is the definition) -> (label[, index][, size],
        n_islands[, stats dict]), without the pairs ever existing.  label: int32[n_items], the smallest slot of each slot's island, the
        same bytes every time; -1 for a dead slot of a dynamic scene; a live slot without a contact is an island of one.  index=True:
        int32[n_items], the islands numbered 0 .. n_islands - 1 in ascending label order (-1 for a dead slot).  sizes=True:
        uint32[n_items], the slots of each slot's island (0 for a dead slot).  n_islands: how many islands there are.  stats: the
        counters of contacts(margin, capacity=0, stats=True) -- the same walk, test for test.  device=False: the host entry, numpy
        results.  device=True: the device entry on `stream` (a torch stream or a hipStream_t as int; default the current torch stream),
        torch tensors on the scene's device -- nothing is waited for, and n_islands is a 0-d int64 tensor."""
        margin = float(margin)
        if margin != margin:
            raise ValueError("margin must not be NaN")
        return self._islands_query("rt_scene_islands", self._side(device=device), False, None, lambda d: (margin,), index, sizes, stats, stream)

    def impact_islands(self, disp, index=False, sizes=False, stats=False, stream=None):
        """rt_scene_impact_islands / rt_scene_impact_islands_device: the connected groups of the impacts of one step -- islands() with the
        pairs impacts(disp) lists as the edges (`disp`: n_items x 3, the scene's REAL dtype, as impacts() takes it): the groups a
        continuous-collision step has to resolve together -> (label[, index][, size], n_islands[, stats dict]) as islands() gives
        them; stats: the counters of impacts(disp, capacity=0, stats=True).  A numpy array goes through the host entry and gives numpy
        results; its components must be finite and within +-1e15.  A torch tensor on this scene's device goes through the device entry
        on `stream` and gives torch tensors -- nothing is waited for, and n_islands is a 0-d int64 tensor."""
        return self._islands_query("rt_scene_impact_islands", self._side(disp), True, disp, lambda d: (d,), index, sizes, stats, stream)

    def swept_overlaps(self, queries, qdisp, disp=None, exclude=None, order=None, capacity=None, times=False, normals=False, offsets=False, stats=False,
                       stream=None):
        """rt_swept_overlaps / rt_swept_overlaps_device: every sphere of the scene that each moving query sphere of `queries` (n x 4: px, py,
        pz, q, the scene's REAL dtype; query g is at p + t qdisp[g] for t in [0, 1], `qdisp`: n x 3) comes into contact with while sphere k of
        the scene moves from c_k to c_k + disp[k] (`disp`: n_items x 3 as impacts() takes it, or None: the scene stands still; swept_times is
        the metric) -> (items[, time][, normal][, offsets], total[, stats dict]).  items: int32[m], the DFS slots of the touched spheres,
        query after query, ascending within a query, the same bytes every time; a dead slot is never listed.  times=True: REAL[m], each
        entry's t in [0, 1] (0: in contact at the start).  normals=True: REAL[m, 3], the unit vector from the touched sphere's centre to the
        query's at contact (swept_normals; NaN where the centres coincide).  offsets=True: uint64[n + 1], query g owns entries offsets[g]
        .. offsets[g + 1].  total: how many entries there are.  capacity, exclude, order (True: sphere_order of the start poses), numpy and
        torch arguments, `stream` and the results' types are overlaps()'s; times and normals need items (not capacity=0).  A query whose q
        is not >= 0 has an empty row; q = 0 is a moving point."""
        if (times or normals) and capacity is not None and int(capacity) == 0:
            raise ValueError("times and normals need items: capacity must not be 0")
        return self._list_query("rt_swept_overlaps", self._side(queries), (queries, qdisp, disp),
                                (("queries", 4, None, False), ("qdisp", 3, _N, False), ("disp", 3, _ITEMS, True)), exclude, order, capacity,
                                (True, times, normals), (((), np.int32), ((), "R"), ((3,), "R")), offsets, stats, stream,
                                "the queries have %d entries", lambda xs, n, ex, o: (xs[0], xs[1], n, xs[2], ex, o))

    def first_contacts(self, queries, qdisp, disp=None, any_hit=False, exclude=None, order=None, normals=False, stats=False, stream=None, out=None):
        """rt_first_contacts / rt_first_contacts_device: the earliest contact of each moving query sphere of `queries` (n x 4: px, py, pz, q;
        query g is at p + t qdisp[g] for t in [0, 1], `qdisp`: n x 3) with the scene while sphere k of the scene moves from c_k to c_k +
        disp[k] (`disp`: n_items x 3, or None: the scene stands still) -- all as swept_overlaps() takes them -> (time[n], item[n][,
        normal[n, 3]][, stats dict]).  There is no metric of its own: swept_times and swept_normals already are the definition -- time is
        swept_times of the (query, item) returned, normal (normals=True) its swept_normals (NaN where the centres coincide at t = 0) --
        and the result is the smallest time of the query's swept_overlaps row, at its lowest slot.  A query that touches nothing during
        the step, or whose q is not >= 0, reads +inf, -1 and a zero normal; q = 0 is a moving point.  any_hit=False (RT_SWEEP_NEAREST):
        the earliest contact, equal times to the first item in DFS order; a query in contact at its start reads 0 and ends its walk
        there.  any_hit=True (RT_SWEEP_ANY): some contact of the step, found sooner.  exclude (int32[n]): the item slot each query never
        returns -- np.arange(n) with the scene's own items, their `disp` as `qdisp`, for the scene against itself; -1 or a slot outside
        the scene excludes nothing.  A dead slot of a dynamic scene is never returned.  numpy arrays go through the host entry, a torch
        tensor on this scene's device through the device entry on `stream`, with the stream discipline of intersect(); out: optional
        (time, item[, normal]) arrays / tensors to fill.  order (uint32[n]): lane j carries query order[j]; the results and counters are
        the same bytes whatever the order, only the time differs.  The host entry wants a permutation; through the device entry an index
        >= n carries no query and leaves that thread's outputs alone."""
        mode = capi.RT_SWEEP_ANY if any_hit else capi.RT_SWEEP_NEAREST
        specs = (((), "R"), ((), np.int32)) + ((((3,), "R"),) if normals else ())
        return self._fixed_query("rt_first_contacts", queries, "queries", 4, (), (), exclude, order, False, specs, out, stats, stream,
                                 lambda x, r, n, ex, o, res, st, stream: (mode, x, r[0], n, r[1], ex, o, *res, *((None,) if not normals else ()), st, *stream),
                                 rows=((qdisp, "qdisp", 3, _N, False), (disp, "disp", 3, _ITEMS, True)))

    def ray_order(self, rays, stream=None):
        """rt_ray_order / rt_ray_order_device: the coherent order of `rays` (n x 6, the scene's REAL dtype), computed on the device -> uint32[n],
        order[j] = the ray lane j should carry: np.argsort(ray_keys(rays), kind="stable").  numpy in, numpy out; a torch tensor on this
        scene's device goes through the device entry on `stream` (as intersect() routes) and gives a torch.uint32 tensor."""
        return self._order_query("rt_ray_order", rays, "rays", 6, None, stream)

    def _camera(self, camera):
        cam = np.asarray(camera)
        R = _real(self.scene.precision)
        if cam.dtype != R or cam.size != 12:
            raise ValueError("camera must be 12 values of %s (eye, right, up, forward; see look_at)" % np.dtype(R).name)
        return np.ascontiguousarray(cam.reshape(12))

    def trace(self, rays, want_stats=False, stream=None, out=None, order=None):
        """rt_trace_rays / rt_trace_rays_device: Renderer::raytrace (render.rs:171-215) for every ray of `rays` (n x 6: pos.xyz, dir.xyz, the
        scene's REAL dtype) -> (color[n, 3], alpha[n][, stats dict]): primary hit, shading and shadow ray, as the render traces a sample.
        numpy arrays go through the host entry (out: optional (color, alpha) arrays to fill, e.g. from capi.HostBuffer); a torch tensor on
        this scene's device goes through the device entry on `stream`, with the stream discipline of intersect().  order (None, True or
        indices; rt_trace_rays_ordered*): as for intersect()."""
        return self._ray_query("rt_trace_rays", (), rays, (), order, (((3,), "R"), ((), "R")), out, want_stats, stream)

    def render_camera(self, options, camera, regions, want_stats=True, out=None):
        """rt_render_camera: render_tiles through a pinhole camera (REAL[12] = eye, right, up, forward; see look_at) -> (uint8[total_px*4]
        tile-major, stats dict | None).  The identity camera of Scene::eye gives render_tiles' bytes."""
        cam = self._camera(camera)
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        nbytes = capi.lib.rt_tiles_rgba_bytes(arr, len(arr))
        if out is None:
            out = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < nbytes:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % nbytes)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_camera(self._h, C.byref(o), cam.ctypes.data, arr, len(arr), out.ctypes.data, C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_camera")
        return out.reshape(-1)[:int(nbytes)], (st.as_dict() if want_stats else None)

    def render_camera_device(self, options, camera, regions, out_ptr, stream=0, want_stats=False):
        """rt_render_camera_device: render_tiles_device through a pinhole camera (host REAL[12]), enqueued on `stream` (hipStream_t as int)."""
        cam = self._camera(camera)
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_camera_device(self._h, C.byref(o), cam.ctypes.data, arr, len(arr), C.c_void_p(out_ptr), C.c_void_p(stream),
                                              C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_camera_device")
        return st.as_dict() if want_stats else None

    def render_camera_undersampled(self, options, camera, regions, step, prev_step=0, want_stats=True, out=None):
        """rt_render_camera_undersampled: the camera frame sampled once per step x step cell of the image's lattice (expand_undersampled is
        its definition) -> (uint8[total_px*4] tile-major, stats dict | None).  prev_step = 2 * step refines `out`, which holds the step-2s
        frame of the same view and regions, in place: only the cells off the 2s lattice are traced and written."""
        cam = self._camera(camera)
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        nbytes = capi.lib.rt_tiles_rgba_bytes(arr, len(arr))
        if out is None:
            if prev_step:
                raise ValueError("a refinement pass (prev_step != 0) needs `out`, the buffer that holds the coarser frame")
            out = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < nbytes:
            raise ValueError("out must be a contiguous uint8 array of at least %d bytes" % nbytes)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_camera_undersampled(self._h, C.byref(o), cam.ctypes.data, arr, len(arr), int(step), int(prev_step), out.ctypes.data,
                                                    C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_camera_undersampled")
        return out.reshape(-1)[:int(nbytes)], (st.as_dict() if want_stats else None)

    def render_camera_undersampled_device(self, options, camera, regions, step, out_ptr, prev_step=0, stream=0, want_stats=False):
        """rt_render_camera_undersampled_device: the same into (prev_step != 0: in) device memory, enqueued on `stream` (hipStream_t as int)."""
        cam = self._camera(camera)
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        st = capi.Stats()
        o = capi.Options(*options)
        rc = capi.lib.rt_render_camera_undersampled_device(self._h, C.byref(o), cam.ctypes.data, arr, len(arr), int(step), int(prev_step),
                                                           C.c_void_p(out_ptr), C.c_void_p(stream), C.byref(st) if want_stats else None)
        capi.check(rc, "rt_render_camera_undersampled_device")
        return st.as_dict() if want_stats else None

    def render_camera_progressive(self, options, camera, regions, first_step=8, out=None):
        """A generator of (step, frame_bytes, stats) for first_step, first_step / 2, ..., 1 over ONE buffer: a coarse frame at once, then
        refinement passes that trace no sample twice; the last frame is render_camera's.  first_step: a power of two <= 64 (ValueError
        otherwise, raised by this call).  Stop iterating when the camera moves; frame_bytes is a view of the buffer the next pass refines."""
        steps = progressive_steps(first_step)

        def passes():
            buf, prev = out, 0
            for s in steps:
                buf, st = self.render_camera_undersampled(options, camera, regions, s, prev_step=prev, out=buf)
                prev = s
                yield s, buf, st
        return passes()

    def blit_tiles_device(self, options, regions, src_ptr, frame_ptr, stream=0, src_px_offset=None):
        """rt_blit_tiles_device: tile-major device tiles -> row-major device frame (set_pixels_from_buffer)."""
        arr = regions if isinstance(regions, C.Array) else self._regions(regions)
        offs = None
        if src_px_offset is not None:
            offs = np.ascontiguousarray(src_px_offset, dtype=np.uint32)
        o = capi.Options(*options)
        rc = capi.lib.rt_blit_tiles_device(self._h, C.byref(o), arr, len(arr), offs.ctypes.data if offs is not None else None,
                                           C.c_void_p(src_ptr), C.c_void_p(frame_ptr), C.c_void_p(stream))
        capi.check(rc, "rt_blit_tiles_device")


class Gang:
    """rt_gang: the Scene replicated on several GPUs of this node in ONE process; a frame's buckets are dealt round-robin over
    them and the u8 shards come back through one RCCL gather (the native twin of dist.FrameSharder's one-process-per-GPU path)."""

    def __init__(self, scene, devices):
        self.scene = scene
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        nb = 0 if scene.bounds is None else scene.bounds.shape[0]
        st = capi.lib.rt_gang_create(devs, len(devices), scene.precision, scene.items.ctypes.data, scene.items.shape[0],
                                     scene.directional_light.ctypes.data, scene.eye.ctypes.data,
                                     scene.bounds.ctypes.data if nb else None, scene.ranges.ctypes.data if nb else None, nb, C.byref(h))
        capi.check(st, "rt_gang_create")
        self._h = h

    def size(self):
        n = C.c_int(0)
        capi.check(capi.lib.rt_gang_size(self._h, C.byref(n)), "rt_gang_size")
        return n.value

    def render_frame(self, options, regions, traversal=capi.RT_TRAVERSAL_SKIP, want_stats=False, out=None):
        """rt_gang_render_frame -> (uint8[h, w, 4] row-major frame, stats dict | None)."""
        arr = regions if isinstance(regions, C.Array) else DeviceScene._regions(regions)
        o = capi.Options(*options)
        if out is None:
            out = np.zeros(o.width * o.height * 4, dtype=np.uint8)
        st = capi.Stats()
        rc = capi.lib.rt_gang_render_frame(self._h, C.byref(o), traversal, arr, len(arr), out.ctypes.data, C.byref(st) if want_stats else None)
        capi.check(rc, "rt_gang_render_frame")
        return out.reshape(o.height, o.width, 4), (st.as_dict() if want_stats else None)

    def render_frames(self, options, regions, n_frames, traversal=capi.RT_TRAVERSAL_SKIP, want_stats=False, out=None):
        """rt_gang_render_frames -> (list of n_frames uint8[h, w, 4] frames, stats dict | None): frame f's gather runs under the
        render of frame f + 1.  out: optional list of contiguous uint8 arrays (pinned ones are written by the root GPU directly)."""
        arr = regions if isinstance(regions, C.Array) else DeviceScene._regions(regions)
        o = capi.Options(*options)
        nbytes = o.width * o.height * 4
        if out is None:
            out = [np.zeros(nbytes, dtype=np.uint8) for _ in range(n_frames)]
        for a in out:
            if a.dtype != np.uint8 or not a.flags.c_contiguous or a.size < nbytes:
                raise ValueError("every frame must be a contiguous uint8 array of at least %d bytes" % nbytes)
        ptrs = (C.c_void_p * n_frames)(*[a.ctypes.data for a in out])
        st = capi.Stats()
        rc = capi.lib.rt_gang_render_frames(self._h, C.byref(o), traversal, arr, len(arr), ptrs, n_frames, C.byref(st) if want_stats else None)
        capi.check(rc, "rt_gang_render_frames")
        return [a.reshape(-1)[:nbytes].reshape(o.height, o.width, 4) for a in out], (st.as_dict() if want_stats else None)

    def close(self):
        if getattr(self, "_h", None):
            capi.lib.rt_gang_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

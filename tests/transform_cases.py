"""Test helper (not a conftest): spheres and meshes under general affine maps.

- MAPS: a named catalogue of affine maps (3 x 3 linear parts at the size of the room's spheres), moderately conditioned: the point
  is the code path a map takes -- the ball short form of the item loop (scene_pack.cpp recognises translation + positive uniform scale)
  or the general SMALL_KIND_SPHERE item, intersect_sphere through a full world_to_object, the normal through its inverse transpose --
  not fp32 conditioning.
- An fp64 numpy reference written from the geometry, not from either implementation: a ray against a transformed unit sphere (solved
  in object space with the fp64 inverse), a ray against triangles (plane, then the point's coordinates in the triangle), and
  `Reference`, the closest hit of a whole Scene by brute force, which also says which rays are GRAZING: those whose answer an fp32
  evaluation may legitimately give differently.
- Scene builders on the 77 x 45 film of kernel_matrix over kernel_matrix.room and its `ctm` keyword, and the probe rays of the
  intersection tests.

test_transform_cases.py checks the catalogue, the packer, the loader and the oracle against this reference on the CPU;
test_gpu_transforms.py the device."""
import numpy as np

import kernel_matrix as km
from rene_amd import abi, glam, scenes
from rene_amd.scene import TriangleMesh

R = 0.3  # the size of a catalogue sphere: kernel_matrix.room's radius


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    return np.asarray(glam.from_axis_angle(a / np.linalg.norm(a), angle), np.float64)[:3, :3]


_ROT = _rot((1.0, 2.0, 3.0), 0.7)
_SHEAR = np.array([[1.0, 0.5, 0.2], [0.0, 1.0, 0.4], [0.0, 0.0, 1.0]])
_CYCLE = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # x -> y -> z -> x: 120 degrees about (1, 1, 1), exact
IN_TOL, OUT_TOL = 2.5e-7, 4e-6  # either side of the recogniser's 1e-6 |r| (scene_pack.cpp)


def _off(rel):
    m = np.eye(3)
    m[1, 1] += rel   # a diagonal entry and an off-diagonal one, both off by `rel` of the radius
    m[1, 0] = rel
    return m


# unit-size linear parts (float64); `linear(name, size)` scales and rounds once to the float32 the ABI carries
_UNIT = {
    "uniform": np.eye(3),                                      # control: recognised as a ball
    "rotated": _ROT,                                           # arbitrary axis
    "nonuniform": _ROT @ np.diag([1.0, 2.0, 0.5]),
    "sheared": _ROT @ _SHEAR,
    "mirrored": _ROT @ np.diag([-1.0, 1.5, 0.8]),              # negative determinant
    "mirrored-uniform": -np.eye(3),                            # uniform, but not r > 0: the general item
    "cyclic": _CYCLE,                                          # the matrix diagonal is exactly zero
    "inside-tolerance": _off(IN_TOL),                          # still a ball
    "outside-tolerance": _off(OUT_TOL),                        # no longer
}
MAPS = tuple(_UNIT)
BALLS = ("uniform", "inside-tolerance")  # what the recogniser takes for translation + positive uniform scale
GENERAL = tuple(n for n in MAPS if n not in BALLS)
MAX_CONDITION = 8.0


def linear(name, size=R):
    return (_UNIT[name] * size).astype(np.float32)


def ctm(name, at=(0.0, 0.0, 0.0), size=R):
    """The 4 x 4 float32 matrix (m[row, col], as rene_amd.glam) of map `name` at size `size`, translated to `at`."""
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = linear(name, size)
    m[:3, 3] = np.asarray(at, np.float32)
    return m


def quirk_radius(m):
    """The reference's sphere-emitter radius (quirk Q4): the mean of the absolute diagonal of object_to_world."""
    m = np.asarray(m, np.float32)
    return float((np.abs(m[0, 0]) + np.abs(m[1, 1]) + np.abs(m[2, 2])) / np.float32(3.0))


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------
TMIN, TMAX = 1e-3, 1e5
T_RTOL = T_ATOL = 5e-5   # the project's margin for t (test_gpu_edge.py, test_box_item_merging_on_random_parallelepipeds)
# GRAZING: a condition on the ray, from the fp64 reference alone, not a tolerance on the answer.
# - sphere: |disc| / half_b^2 < GRAZING_DISC.  fp32 evaluates disc = half_b^2 - a c with an error of ~ 2e-6 half_b^2 (eight roundings of
#   6e-8 and the cancellation of the translation in world_to_object . o at 1 / 0.15 of the room's coordinates); the root moves by
#   d(disc) / (2 sqrt(disc)), i.e. by 2e-6 / (2 sqrt(1e-3)) = 3e-5 of half_b / a at the threshold, inside the margin for t -- and
#   below it hit and miss may swap
# - sphere: the two roots within ROOT_GAP of each other, whatever half_b is (a ray that starts ON the surface has half_b^2 = disc, and
#   leaves within 1 degree of the tangent plane when its chord is that short): fp32 has c = |oc|^2 - 1 to ~ 1e-6, the roots take it over
#   a gap: 1e-6 / (11 . 1e-2) = 1e-5 at a = 1 / 0.3^2, a fifth of the margin
# - a root within twice the margin of tmin
# - triangle: the hit point within EDGE of an edge in the triangle's own coordinates (the project's atol for u and v is 2e-4), or the
#   cosine between ray and normal below PARALLEL: fp32 places the origin against the plane to ~ 5e-7 (eight roundings at the room's
#   coordinates of up to 3), and t takes that over the cosine: 5e-5, the margin, at 1e-2.  A thin triangle's plane is no better than its
#   corners (2e-7 each) over its smallest height: PARALLEL grows by half the longest edge over that height (a needle of 0.118 x 0.003
#   at the pole of a latitude-longitude mesh, met at cos 0.02, moved the device's t by 2e-4 and the oracle's by 3e-5)
# - a second surface within twice the margin behind the closest one (instance and primitive of a tie are anyone's)
GRAZING_DISC = 1e-3
ROOT_GAP = 1e-2
EDGE = 2e-4
PARALLEL = 1e-2


def margin(t):
    return T_ATOL + T_RTOL * np.abs(t)


def ray_sphere(m, o, d, tmin=TMIN, tmax=TMAX):
    """Rays o + t d (float64, (n, 3)) against the unit sphere under the 4 x 4 map m.  Returns (t, normal, disc_n, roots): t is the first
    root in [tmin, tmax], otherwise the second, NaN for a miss; normal the world normal DIRECTION M^-T p at the hit (not normalised);
    disc_n the discriminant over half_b^2; roots (n, 2), NaN where there are none."""
    m = np.asarray(m, np.float64)
    inv = np.linalg.inv(m[:3, :3])
    oc = (o - m[:3, 3]) @ inv.T
    od = d @ inv.T
    a, half_b, c = (od * od).sum(1), (oc * od).sum(1), (oc * oc).sum(1) - 1.0
    disc = half_b * half_b - a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(disc)  # NaN for a miss
        roots = np.stack([(-half_b - sq) / a, (-half_b + sq) / a], 1)
        ok = (roots >= tmin) & (roots <= tmax)
        t = np.where(ok[:, 0], roots[:, 0], np.where(ok[:, 1], roots[:, 1], np.nan))
        disc_n = np.where(half_b != 0.0, disc / (half_b * half_b), np.copysign(np.inf, disc))
    p = oc + np.nan_to_num(t)[:, None] * od
    return t, p @ inv, disc_n, roots


class TriangleSet:
    """m triangles given by their world-space corners (m, 3, 3), float64."""

    def __init__(self, corners):
        p = np.asarray(corners, np.float64)
        self.p0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        self.n = np.cross(e1, e2)  # the geometric normal, |n| = twice the area
        n2 = (self.n * self.n).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            # a point h of the plane is p0 + u e1 + v e2 with u = (h - p0) . gu, v = (h - p0) . gv
            self.gu = np.cross(e2, self.n) / n2[:, None]
            self.gv = np.cross(self.n, e1) / n2[:, None]
            self.unit_n = self.n / np.sqrt(n2)[:, None]
            longest = np.sqrt(np.maximum(np.maximum((e1 * e1).sum(1), (e2 * e2).sum(1)), ((e2 - e1) ** 2).sum(1)))
            self.thin = np.maximum(1.0, 0.5 * longest * longest / np.sqrt(n2))  # half the longest edge over the smallest height
        self.live = n2 > 0.0  # a degenerate triangle is never hit

    def hits(self, o, d):
        """(t, u, v, cos) of every ray against every triangle's PLANE, (n, m) each; cos = d^ . n^."""
        with np.errstate(invalid="ignore", divide="ignore"):
            dn = d @ self.n.T
            t = ((self.p0 * self.n).sum(1) - o @ self.n.T) / dn
            u = o @ self.gu.T - (self.p0 * self.gu).sum(1) + t * (d @ self.gu.T)
            v = o @ self.gv.T - (self.p0 * self.gv).sum(1) + t * (d @ self.gv.T)
            cos = (d @ self.unit_n.T) / np.linalg.norm(d, axis=1)[:, None]
        return t, u, v, cos


def ray_triangles(corners, o, d, tmin=TMIN, tmax=TMAX):
    """The closest of the triangles `corners` (m, 3, 3) per ray: (t, u, v, index, normal), t NaN for a miss; u and v are the weights
    of the second and third corner, normal the geometric one (e1 x e2, not normalised)."""
    ts = TriangleSet(corners)
    t, u, v, _ = ts.hits(o, d)
    inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax) & ts.live
    t = np.where(inside, t, np.inf)
    k = t.argmin(1)
    r = np.arange(len(o))
    miss = ~np.isfinite(t[r, k])
    return np.where(miss, np.nan, t[r, k]), u[r, k], v[r, k], np.where(miss, -1, k), ts.n[k]


def world_corners(scene, inst):
    """(m, 3, 3) float64: the corners of a triangle instance in world space, from the float32 numbers the ABI carries."""
    mesh = scene.meshes[inst.mesh_index]
    a = np.asarray(inst.matrix[:], np.float64)
    lin, tr = a[:9].reshape(3, 3).T, a[9:12]
    p = mesh.vertices[:, 0:3].astype(np.float64) @ lin.T + tr
    return p[mesh.indices.reshape(-1, 3).astype(np.int64)]


def instance_matrix(inst):
    a = np.asarray(inst.matrix[:], np.float64)
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = a[:9].reshape(3, 3).T, a[9:12]
    return m


class Reference:
    """The closest hit of a Scene by brute force in fp64.  which = 1: the emitter structure (the instances with an area light)."""

    def __init__(self, scene, which=0):
        self.spheres, self.meshes = [], []
        for i, inst in enumerate(scene.instances):
            if which and not inst.area_light_index:
                continue
            if inst.shape == abi.SHAPE_SPHERE:
                self.spheres.append((i, instance_matrix(inst)))
            else:
                self.meshes.append((i, TriangleSet(world_corners(scene, inst))))

    def trace(self, origins, directions, tmin=TMIN, tmax=TMAX, chunk=1024):
        o = np.asarray(origins, np.float32).reshape(-1, 3).astype(np.float64)
        d = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
        n = len(o)
        out = {"t": np.full(n, np.inf), "u": np.zeros(n), "v": np.zeros(n), "instance": np.full(n, -1), "primitive": np.full(n, -1),
               "normal": np.zeros((n, 3))}
        second = np.full(n, np.inf)    # the closest surface that is not the hit
        graze = np.full(n, np.inf)     # the smallest ray parameter at which something ill-conditioned happens

        def take(rows, t, u, v, inst, prim, normal):
            """candidates (t = inf: none) for the rays `rows`"""
            better = t < out["t"][rows]
            second[rows] = np.where(better, np.minimum(second[rows], out["t"][rows]), np.minimum(second[rows], t))
            w = rows[better]
            for k, val in (("t", t), ("u", u), ("v", v), ("instance", inst), ("primitive", prim)):
                out[k][w] = (val[better] if isinstance(val, np.ndarray) else val)
            out["normal"][w] = normal[better]

        everyone = np.arange(n)
        for i, m in self.spheres:
            t, normal, disc_n, roots = ray_sphere(m, o, d, tmin, tmax)
            inv = np.linalg.inv(m[:3, :3])
            oc, od = (o - m[:3, 3]) @ inv.T, d @ inv.T
            nearest = -(oc * od).sum(1) / (od * od).sum(1)  # the ray parameter of the closest approach
            with np.errstate(invalid="ignore"):
                ill = ((np.abs(disc_n) < GRAZING_DISC) | (roots[:, 1] - roots[:, 0] < ROOT_GAP)) & (nearest > tmin - ROOT_GAP) & (nearest < tmax)
                graze[ill] = np.minimum(graze[ill], np.fmin(nearest, t)[ill])
                edge = (np.abs(roots - tmin) < 2 * margin(tmin)).any(1)
                graze[edge] = -np.inf
            take(everyone, np.where(np.isnan(t), np.inf, t), 0.0, 0.0, i, 0, normal)
        for i, ts in self.meshes:
            for lo in range(0, n, chunk):
                rows = everyone[lo:lo + chunk]
                t, u, v, cos = ts.hits(o[rows], d[rows])
                w = 1.0 - u - v
                with np.errstate(invalid="ignore"):
                    low = np.minimum(np.minimum(u, v), w)
                    valid = (t >= tmin) & (t <= tmax) & ts.live
                    inside = valid & (low >= 0.0)
                    near = ts.live & (t > tmin - 1e-3) & (t <= tmax) & (low >= -EDGE)
                    ill = near & ((low <= EDGE) | (np.abs(cos) < PARALLEL * ts.thin) | (np.abs(t - tmin) < 1e-3))
                graze[rows] = np.minimum(graze[rows], np.where(ill, t, np.inf).min(1))
                t = np.where(inside, t, np.inf)
                k = t.argmin(1)
                r = np.arange(len(rows))
                tk = t[r, k].copy()
                t[r, k] = np.inf
                runner_up = t.min(1)  # (two triangles of one mesh tie along their shared edge, which EDGE covers, and where they coincide)
                take(rows, tk, u[r, k], v[r, k], i, k, ts.n[k])
                second[rows] = np.minimum(second[rows], runner_up)
        hit = np.isfinite(out["t"])
        reach = np.where(hit, out["t"] + 2 * margin(np.where(hit, out["t"], 0.0)), np.inf)
        out["grazing"] = ((graze < np.inf) & (graze <= reach)) | (hit & (second <= reach))
        out["t"] = np.where(hit, out["t"], -1.0)
        return out


def compare_hits(got, ref, what=""):
    """`got` (a rene_hit array of the device or the oracle) against Reference.trace: hit or miss, instance and primitive equal and t
    within the margin on every ray that is not grazing.  Returns the number of rays compared."""
    keep = ~ref["grazing"]
    miss_g, miss_r = got["t"] < 0, ref["t"] < 0
    wrong = keep & (miss_g != miss_r)
    assert not wrong.any(), (what, "hit / miss", int(wrong.sum()), np.nonzero(wrong)[0][:8])
    both = keep & ~miss_r
    for k in ("instance", "primitive"):
        wrong = both & (got[k].astype(np.int64) != ref[k])
        assert not wrong.any(), (what, k, int(wrong.sum()), np.nonzero(wrong)[0][:8])
    err = np.abs(got["t"][both].astype(np.float64) - ref["t"][both])
    over = err > margin(ref["t"][both])
    assert not over.any(), (what, "t", int(over.sum()), float(err.max()), np.nonzero(both)[0][over][:8])
    return int(keep.sum())


def triangle_emitter_pdf(ref, directions, n_triangles):
    """The reference's pdf of a triangle emitter's hit (triangle_closest_hit_pdf) in fp64, from Reference.trace's hit: distance^2 over
    |cos| times the world-space area, over the emitter's triangle count.  NaN for a miss."""
    d = np.asarray(directions, np.float64)
    length = np.linalg.norm(ref["normal"], axis=1)  # twice the area
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.abs((ref["normal"] * d).sum(1)) / (length * np.linalg.norm(d, axis=1))
        pdf = (ref["t"] * np.linalg.norm(d, axis=1)) ** 2 / (cos * 0.5 * length) / n_triangles
    return np.where(ref["t"] > 0, pdf, np.nan)


def compare_points(got, ref, scene):
    """The point of the triangle that `got`'s u and v name against the reference's, on the rays compare_hits has passed: within the
    margin for t (an error of the plane's distance moves t by it over the cosine and the point in the plane by its tangent times as
    much: less).  u and v themselves are as ill-conditioned as the triangle is thin."""
    keep = ~ref["grazing"] & (ref["t"] > 0)
    n = 0
    for i, inst in enumerate(scene.instances):
        rows = np.nonzero(keep & (ref["instance"] == i))[0]
        if inst.shape != abi.SHAPE_TRIANGLE or not len(rows):
            continue
        c = world_corners(scene, inst)[ref["primitive"][rows]]
        point = lambda h: c[:, 0] + np.asarray(h["u"][rows], np.float64)[:, None] * (c[:, 1] - c[:, 0]) + \
            np.asarray(h["v"][rows], np.float64)[:, None] * (c[:, 2] - c[:, 0])
        err = np.linalg.norm(point(got) - point(ref), axis=1)
        assert (err <= margin(ref["t"][rows])).all(), (i, float(err.max()), rows[err.argmax()])
        n += len(rows)
    return n


# ---- probe rays -----------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _to_world(m, p_obj):
    return p_obj @ m[:3, :3].T + m[:3, 3]


def sphere_rays(m, rng, n):
    """n rays for the sphere under the 4 x 4 map m, built in its object space and carried to the world: 55 % aimed from outside at a
    ball 1.1 times the sphere (hits and near misses), 25 % started inside (the second root), 19.5 % started on the surface, inwards
    and outwards (the first root at 0 < tmin), 0.5 % tangent.  float32 (origins, unit directions)."""
    m = np.asarray(m, np.float64)
    n_tan = max(1, n // 200)
    n_out, n_in = int(0.55 * n), int(0.25 * n)
    n_on = n - n_out - n_in - n_tan
    o_out = _unit(rng, n_out) * rng.uniform(1.5, 3.0, (n_out, 1))
    t_out = _unit(rng, n_out) * (1.1 * rng.random((n_out, 1)) ** (1 / 3))
    o_in = _unit(rng, n_in) * (0.8 * rng.random((n_in, 1)) ** (1 / 3))
    t_in = o_in + _unit(rng, n_in)
    o_on = _unit(rng, n_on)
    t_on = o_on + _unit(rng, n_on)
    p = _unit(rng, n_tan)
    tau = np.cross(p, _unit(rng, n_tan))
    tau /= np.linalg.norm(tau, axis=1, keepdims=True)
    o_tan = p - tau * rng.uniform(1.0, 3.0, (n_tan, 1))
    o = _to_world(m, np.concatenate([o_out, o_in, o_on, o_tan])).astype(np.float32)
    tgt = _to_world(m, np.concatenate([t_out, t_in, t_on, p]))
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def mesh_rays(corners, rng, n):
    """n rays from points of the room at points of the triangles `corners` (m, 3, 3), through them from either side."""
    k = rng.integers(0, len(corners), n)
    b = rng.random((n, 2))
    flip = b.sum(1) > 1
    b[flip] = 1 - b[flip]
    tgt = corners[k, 0] + b[:, :1] * (corners[k, 1] - corners[k, 0]) + b[:, 1:] * (corners[k, 2] - corners[k, 0])
    o = np.stack([rng.uniform(-2.4, 2.4, n), rng.uniform(0.05, 2.4, n), rng.uniform(-2.4, 2.4, n)], 1).astype(np.float32)
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def probe_rays(scene, seed, per_sphere=1400, per_mesh=600):
    """The ray set of the intersection tests: sphere_rays for every sphere, mesh_rays for every mesh instance."""
    rng = np.random.default_rng(seed)
    o, d = [], []
    for inst in scene.instances:
        if inst.shape == abi.SHAPE_SPHERE:
            a, b = sphere_rays(instance_matrix(inst), rng, per_sphere)
        else:
            a, b = mesh_rays(world_corners(scene, inst), rng, per_mesh)
        o.append(a)
        d.append(b)
    return np.concatenate(o), np.concatenate(d)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def smooth_displaced_sphere(n_lat, n_lon, radius, amplitude, seed):
    """scenes.displaced_sphere with vertex normals: the area-weighted mean of the geometric normals of a vertex's triangles (the
    seam's two copies of a vertex get their own; every normal is far from zero)."""
    mesh = scenes.displaced_sphere(n_lat, n_lon, radius=radius, amplitude=amplitude, seed=seed)
    p = mesh.vertices[:, 0:3].astype(np.float64)
    idx = mesh.indices.reshape(-1, 3).astype(np.int64)
    fn = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    vn = np.zeros_like(p)
    for k in range(3):
        np.add.at(vn, idx[:, k], fn)
    vn /= np.linalg.norm(vn, axis=1, keepdims=True)
    return TriangleMesh.from_arrays(mesh.vertices[:, 0:3], mesh.indices, normals=vn.astype(np.float32))


def bumpy_octahedron(seed, smooth):
    """Eight well-shaped triangles: an octahedron of radius ~ 0.4 with its corners moved at random; with `smooth`, vertex normals
    (the area-weighted mean of a corner's faces), else none.  (The poles of a coarse scenes.displaced_sphere are needles, whose plane
    fp32 places no better than 1e-5 rad: conditioning, which these tests are not about.)"""
    rng = np.random.default_rng(seed)
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.4 + rng.uniform(-0.08, 0.08, (6, 3))
    idx = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    if not smooth:
        return TriangleMesh.from_arrays(p, idx.reshape(-1))
    fn = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    vn = np.zeros_like(p)
    for k in range(3):
        np.add.at(vn, idx[:, k], fn)
    return TriangleMesh.from_arrays(p, idx.reshape(-1), normals=vn / np.linalg.norm(vn, axis=1, keepdims=True))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
SPHERE_Y = 0.65  # a catalogue sphere reaches 0.6 from its centre at most (`nonuniform`): clear of the floor


def placed(kinds, name, boxes=True, deep=None):
    """kernel_matrix.room's `ctm` for `kinds`: every sphere under map `name` where room puts it (lifted clear of the floor), every box
    under the same map at twice the size (a 0.6 x 0.9 x 0.5 block before the map), the deep mesh under map `deep`."""
    out = {}
    for i in range(len(kinds)):
        x = -1.5 + 3.0 * (i + 0.5) / len(kinds)
        out["sphere", i] = ctm(name, (x, SPHERE_Y, -0.6))
        if boxes:
            out["box", i] = ctm(name, (x, 1.0, 1.3), size=1.0 if name not in ("nonuniform",) else 0.6)
    if deep:
        out["deep"] = ctm(deep, (0.5, 0.75, 0.2), size=0.7 if deep == "nonuniform" else 1.0)
    return out


def gallery(deep=False, emissive=True):
    """Every map of the catalogue on one sphere each (emitters all, with `emissive`), in three rows above kernel_matrix.room's floor;
    a box under `sheared`, a flat bumpy_octahedron under `mirrored` and a smooth one under `nonuniform`: few enough
    items for the item loop; with `deep` the room's 3 520-triangle mesh under `sheared`: a main BVH of more than 512 nodes."""
    s = km.room(deep="matte" if deep else None, ctm={"deep": ctm("sheared", (0.5, 0.62, 0.2), size=0.8)})
    grey = s.add_matte((0.5, 0.5, 0.5))
    al = s.add_area_light_diffuse((2.0, 2.0, 2.0)) if emissive else 0
    for k, name in enumerate(MAPS):
        s.add_sphere(1.0, grey, area_light=al, ctm=ctm(name, (-1.5 + 1.5 * (k % 3), 1.6, -1.5 + 1.3 * (k // 3))))
    s.add_triangle_mesh(scenes._aabb((-0.3, -0.45, -0.25), (0.3, 0.45, 0.25)), grey, ctm=ctm("sheared", (-1.7, 0.6, 0.3), size=0.8))
    s.add_triangle_mesh(bumpy_octahedron(3, False), grey, ctm=ctm("mirrored", (1.6, 0.7, -1.2), size=0.8))
    s.add_triangle_mesh(bumpy_octahedron(4, True), grey, ctm=ctm("nonuniform", (-0.6, 0.6, -1.6), size=0.6))
    return s


TEXELS = np.random.default_rng(5).random((5, 7, 3), dtype=np.float32)  # as test_image_map_repeats_over_many_periods


def first_hit_spheres(name):
    """The room with three spheres under map `name` -- Matte over a 7 x 5 image map (the albedo layer shows sphere_uv), Glass, Mirror --
    and their boxes under the same map."""
    kinds = ("image", "glass", "mirror")
    return km.room(kinds, spheres=True, ctm=placed(kinds, name))


def first_hit_mesh(name, smooth):
    """The room with a 3 520-triangle displaced sphere under map `name`, with vertex normals (`smooth`) or without (the geometric
    normal through the inverse transpose), Matte over the image map, and a Metal box under the same map."""
    s = km.room(("metal",), ctm=placed(("metal",), name))
    mesh = smooth_displaced_sphere(40, 44, 0.5, 0.12, 5) if smooth else scenes.displaced_sphere(40, 44, radius=0.5, amplitude=0.12, seed=5)
    s.add_triangle_mesh(mesh, s.add_matte((0.6, 0.55, 0.5)), ctm=ctm(name, (0.3, 0.9, -0.4), size=0.7 if name == "nonuniform" else 1.0))
    return s


def emitter_room(name, size=None):
    """A Matte room lit by one sphere emitter under map `name` (and nothing else): small enough for the item loop."""
    s = km.room(emitter=None)
    al = s.add_area_light_diffuse((6.0, 5.5, 4.5))
    s.add_sphere(1.0, s.add_matte((0, 0, 0)), area_light=al, ctm=ctm(name, EMITTER_AT, size=size or EMITTER_SIZE))
    s.add_triangle_mesh(scenes._aabb((-1.2, 0.0, 0.4), (-0.6, 0.8, 1.0)), s.add_matte((0.6, 0.6, 0.55)))
    return s


EMITTER_AT, EMITTER_SIZE = (0.2, 1.5, -0.3), 0.4


def emitter_rays(m, rng, n, far=2.2):
    """Rays at the sphere emitter under the 4 x 4 map m: origins 0.9 .. `far` world units from its centre (outside it: a catalogue map
    at EMITTER_SIZE reaches 0.8 at most), aimed at points inside the ellipsoid."""
    m = np.asarray(m, np.float64)
    o = (m[:3, 3] + _unit(rng, n) * rng.uniform(0.9, far, (n, 1))).astype(np.float32)
    tgt = _to_world(m, _unit(rng, n) * (0.9 * rng.random((n, 1)) ** (1 / 3)))
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def mesh_emitter_room(name, which):
    """A Matte room lit by an emissive quad (`which` "quad") or an emissive 3 520-triangle displaced sphere ("mesh") under map `name`."""
    s = km.room(emitter=None)
    al = s.add_area_light_diffuse((9.0, 8.0, 6.0) if which == "quad" else (3.0, 2.6, 2.0))
    black = s.add_matte((0, 0, 0))
    if which == "quad":  # (a triangle emits on its front side only: the mirrored map turns the quad over, so it is wound the other way)
        p = [[-.5, 0, -.5], [.5, 0, -.5], [.5, 0, .5], [-.5, 0, .5]]
        quad = km._quad(p[::-1] if name.startswith("mirrored") else p)
        s.add_triangle_mesh(quad, black, area_light=al, ctm=ctm(name, (0.0, 2.0, 0.0), size=0.6 if name == "nonuniform" else 1.0))
    else:
        ball = scenes.displaced_sphere(40, 44, radius=0.45, amplitude=0.1, seed=9)
        if not name.startswith("mirrored"):  # (displaced_sphere winds its triangles inwards; a mirror turns them over)
            ball.indices = np.ascontiguousarray(ball.indices.reshape(-1, 3)[:, ::-1].reshape(-1))
        s.add_triangle_mesh(ball, black, area_light=al, ctm=ctm(name, (-0.4, 1.5, 0.6), size=0.6 if name == "nonuniform" else 0.9))
    s.add_triangle_mesh(scenes._aabb((0.6, 0.0, 0.4), (1.2, 0.8, 1.0)), s.add_matte((0.6, 0.6, 0.55)))
    return s


def instanced():
    """One 12 x 14 displaced sphere added once, then instanced twice more with add_mesh_instance under other maps and materials (Matte,
    Metal, Substrate), in the room."""
    s = km.room()
    mesh = smooth_displaced_sphere(12, 14, 0.4, 0.12, 6)
    first = s.add_triangle_mesh(mesh, s.add_matte((0.3, 0.5, 0.7)), ctm=ctm("nonuniform", (-1.2, 0.7, 0.0), size=0.7))
    mi = s.instances[first].mesh_index
    ids = [first,
           s.add_mesh_instance(mi, km._material(s, "metal"), ctm=ctm("sheared", (0.0, 0.7, 0.3), size=0.9)),
           s.add_mesh_instance(mi, km._material(s, "substrate"), ctm=ctm("mirrored", (1.2, 0.7, -0.2), size=0.9))]
    return s, ids


def _matrix_case(entry, name, deep=None):
    """A catalogue scene of kernel_matrix with its spheres and boxes under map `name` (its deep mesh under `deep`)."""
    src = {"metal+spheres": (["metal"], {}),
           "glass-mirror+spheres": (["glass", "mirror"], {}),
           "metal+spheres+sun": (["metal", "image"], dict(sun=True)),
           "plastic-uber": (["plastic", "uber", "image"], dict(sun=True, sky=True, textures=True)),
           "metal-deep+spheres+sun": (["metal", "image"], dict(deep="metal", sun=True)),
           "plastic-uber-deep": (["plastic", "uber", "image"], dict(deep="uber", sun=True, sky=True, textures=True)),
           "fog+glass": (["glass"], dict(volpath=True)),
           "fog+plastic": (["plastic"], dict(volpath=True, sun=True)),
           "fog-deep+substrate+glass": (["glass"], dict(deep="substrate", volpath=True)),
           "fog-deep+uber": (["plastic"], dict(deep="uber", volpath=True, sun=True))}[entry]
    kinds, kw = src
    return lambda: km.room(kinds, spheres=True, ctm=placed(kinds, name, boxes=not kw.get("volpath"), deep=deep if kw.get("deep") else None), **kw)


# a general-sphere scene on every leaf of the dispatch that has FEAT_SPHERES: the catalogue entries of kernel_matrix that carry spheres,
# their spheres, boxes and deep meshes under a map each (Matte over the image map where the leaf has textures)
RENDERS = tuple(km.Entry(f"{e}/{m}", km.BY_NAME[e].family, km.BY_NAME[e].leaf, km.BY_NAME[e].cls, _matrix_case(e, m, d)) for e, m, d in (
    ("metal+spheres", "nonuniform", None),
    ("glass-mirror+spheres", "mirrored", None),
    ("metal+spheres+sun", "rotated", None),
    ("plastic-uber", "sheared", None),
    ("metal-deep+spheres+sun", "sheared", "mirrored"),
    ("plastic-uber-deep", "nonuniform", "sheared"),
    ("fog+glass", "rotated", None),
    ("fog+plastic", "sheared", None),
    ("fog-deep+substrate+glass", "rotated", "mirrored"),
    ("fog-deep+uber", "mirrored", "nonuniform")))
RENDER_BY_NAME = {e.name: e for e in RENDERS}


# ---- what fp32 does to the reference's own formulas ---------------------------------------------------------------------------------
# The oracle rendered twice, as compiled for the parity tests and with its multiply-adds contracted (test_oracle_fp_sensitivity.py's
# build: what a GPU compiler does, a perturbation no larger than the device's): the pixels of the 77 x 45 film that then differ
# (T1: beyond 1e-2 (1 + ref); first-hit normal and albedo: beyond 5e-5 x frames).  Measured on the CPU and recorded here;
# test_transform_cases.py measures again.  Every scene of the new render tests that is not listed measured (0, 0, 0) or a single pixel.
# - A sphere's first-hit normal is ill-conditioned towards its limb: the hit point comes from the small root of a quadratic whose
#   discriminant cancels, at 5 / 0.15 object units from the camera under `nonuniform`, and the inverse transpose stretches what is
#   left by the map's condition (4): 61 pixels of one frame, against 8 for the ball.
# - A sphere emitter is sampled ON its surface and then met by a ray (surface_sample.rs, lib.rs:301-318): a sample near the limb as
#   seen from the shading point is a tangent ray, hit or miss by a rounding, pdf_l or 0.  20 to 29 pixels of 16 frames move beyond T1
#   for the translated ball as for any map; none where pdf_l is infinite (`cyclic`) and the branch weighs nothing.
SELF_FIRST_HIT = {"uniform": (8, 9), "rotated": (10, 4), "nonuniform": (61, 44), "sheared": (9, 6), "mirrored": (26, 7),
                  "mirrored-uniform": (8, 7), "cyclic": (3, 2), "inside-tolerance": (11, 12), "outside-tolerance": (10, 4)}  # one frame
SELF_RENDERS = {"metal+spheres/nonuniform": (0, 17, 0), "plastic-uber-deep/nonuniform": (0, 42, 9), "metal-deep+spheres+sun/sheared": (0, 3, 3),
                "fog+glass/rotated": (12, 0, 0), "fog-deep+substrate+glass/rotated": (11, 0, 0)}  # 16 frames
SELF_EMITTERS = {"uniform": (20, 0, 0), "rotated": (28, 0, 0), "nonuniform": (29, 13, 0), "mirrored": (20, 2, 0), "cyclic": (0, 0, 0)}  # 16 frames


def pixel_bound(measured, project_frac, pixels=km.W * km.H):
    """How many pixels may differ: the project's fraction, or twice what the oracle's two builds differ in plus the kernel matrix's
    floor of 4 (device and oracle are two fp32 evaluations as those are; the count of pixels that cross a threshold scatters by its
    square root), whichever is more.  As a fraction of the film."""
    return max(project_frac, (2 * measured + 4) / pixels)
